#!/usr/bin/env python
"""Mesh evaluation script: render a mesh file from the cameras of a dataset split and score it against the split's images.

The mesh is a PLY that `mesh.write_ply` wrote (extract_mesh.py's output): with per-face texture coordinates it is rendered with the
PNG its `comment TextureFile` line names (looked up next to the file), otherwise with its vertex colours, otherwise as shaded
normals.  Where the header also names a `comment TextureSH` file (extract_mesh.py --texture_sh) and it lies next to the mesh, every
pixel is shaded with the texel's spherical harmonics at its own view direction (`ops.shtex_shade`, csrc/shtex.hip), and the script
says so; --no_view_dependent scores the plain texture instead.  Every view is rendered on the device (`mesh.render_mesh`) and scored
by `image.MetricHarness` (PSNR and SSIM), honouring Config.eval_quantize_metrics and Config.eval_crop_borders as eval.py does.  No
checkpoint is needed.

--method auto|raster|raycast (default auto).  `raster` is the rasteriser (csrc/raster.hip), for undistorted pinhole cameras only: a
dataset whose cameras `mesh.world_to_pixel` refuses fails with its message.  `raycast` casts the dataset's own ray of every pixel at
the mesh (csrc/meshray.hip) and so renders any camera model: lens distortion, a fisheye camtype, an NDC ray space (the rays are taken
in world space, before the NDC conversion) and the spherical 'pano' render camera.  `auto` rasterises a pinhole dataset, with every
output file byte for byte what `raster` writes, and casts rays otherwise; the script prints which method the run used.  A render
path (Config.render_path = True, the only way to a Config.render_camtype) has no images to score: its views are rendered and
written, and the metric files are left out.

Under --out_dir (default: <mesh file's directory>/mesh_eval) it writes mesh_color_NNN.png for every view and, in eval.py's format
(one line, values separated by blanks), mesh_metric_psnr.txt, mesh_metric_ssim.txt and mesh_render_times.txt (seconds a view:
visibility and shading, bracketed by a device synchronisation).

  python eval_mesh.py --mesh garden.ply --gin_configs configs/360.gin --gin_bindings "Config.data_dir = '...'" --supersample 2

Geometry.  With --gt_mesh FILE (a PLY mesh or point cloud, `mesh.read_ply_geometry`) the mesh is also scored against that ground truth
by `mesh.geometry_metrics` (csrc/meshdist.hip): accuracy, completeness, Chamfer, their medians, and precision, recall and F-score at
every threshold, printed as `name = value` and written to mesh_metric_geometry.txt (one `name value` a line), followed by the
seconds of sampling, grid build and the two queries.  --gt_transform FILE holds the 16 numbers of the 4 x 4 matrix from the mesh's
frame to the ground truth's; --geometry_samples, --geometry_thresholds a,b,..., --geometry_max_dist and --geometry_bbox
x0,y0,z0,x1,y1,z1 are geometry_metrics' arguments.  --error_ply FILE writes the mesh with its vertices coloured by their distance to
the ground truth (turbo, 0 .. the largest threshold).  --geometry_only skips the dataset and the rendering: no config is needed.

The Tanks and Temples protocol.  --gt_crop FILE.json is the benchmark's crop volume (a polygonal prism, `mesh.CropVolume.from_json`):
samples of both shapes outside it are dropped.  --icp point|plane refines --gt_transform (or the identity) by `mesh.register`
(csrc/meshreg.hip) before scoring: --icp_max_dist a[,b,c] are the correspondence distances of its stages, coarse to fine (required
with --icp), --icp_iters the updates a stage, --icp_samples the surface samples, --icp_scale estimates a scale too (point only).  It
prints fitness and RMSE of every stage and the seconds of the registration, writes the refined matrix to
mesh_gt_transform_refined.txt (four rows of four numbers) and scores, and colours --error_ply, with it.  --geometry_normals adds the
normal consistency.  There is no voxel down-sampling, no alignment from camera trajectories and no global registration: the
transform given must already be close.

  python eval_mesh.py --mesh barn.ply --geometry_only --gt_mesh Barn.ply --gt_transform Barn_trans.txt --geometry_thresholds 0.01
  python eval_mesh.py --mesh barn.ply --geometry_only --gt_mesh Barn.ply --gt_transform Barn_trans.txt --gt_crop Barn.json \
      --icp point --icp_scale --icp_max_dist 0.15,0.05,0.02 --geometry_thresholds 0.01
"""

import argparse
import os
import sys
import time

import numpy as np
import torch

from multinerf_amd import configs, datasets, image, mesh


def parse_args(argv):
  ap = argparse.ArgumentParser()
  ap.add_argument('--mesh', required=True, help='a PLY file written by mesh.write_ply / extract_mesh.py')
  ap.add_argument('--gin_configs', action='append', default=[])
  ap.add_argument('--gin_bindings', action='append', default=[])
  ap.add_argument('--preset', default=None)
  ap.add_argument('--split', choices=('train', 'test'), default='test', help='the cameras and images to score against')
  ap.add_argument('--out_dir', default=None, help='default: <directory of --mesh>/mesh_eval')
  ap.add_argument('--supersample', type=int, default=1, help='render k x k samples a pixel and box-average them')
  ap.add_argument('--near', type=float, default=None, help='surface nearer than this (zc) is not seen; default: Config.near')
  ap.add_argument('--bg', default='1,1,1', help='r,g,b of the pixels no face covers')
  ap.add_argument('--cull', choices=('none', 'back'), default='none')
  ap.add_argument('--method', choices=('auto', 'raster', 'raycast'), default='auto',
                  help='rasterise (pinhole cameras only), cast rays (any camera model), or choose by the dataset\'s cameras')
  ap.add_argument('--no_view_dependent', action='store_true',
                  help='score the plain texture although the mesh names a `comment TextureSH` file (spherical harmonics per texel)')
  ap.add_argument('--gt_mesh', default=None, help='a ground-truth PLY (mesh or point cloud): score the geometry against it')
  ap.add_argument('--gt_transform', default=None, help='a text file of 16 numbers: the 4 x 4 matrix from the mesh\'s frame to the ground truth\'s')
  ap.add_argument('--geometry_samples', type=int, default=1_000_000, help='surface samples a shape')
  ap.add_argument('--geometry_thresholds', default=None, help='a,b,...: distances of precision / recall / F-score; default: from the ground truth\'s box')
  ap.add_argument('--geometry_max_dist', type=float, default=None, help='distances are clamped to this')
  ap.add_argument('--geometry_bbox', default=None, help='x0,y0,z0,x1,y1,z1 in the ground truth\'s frame: samples outside are dropped')
  ap.add_argument('--geometry_only', action='store_true', help='skip the dataset and the rendering (no config needed)')
  ap.add_argument('--error_ply', default=None, help='write the mesh coloured by its vertices\' distance to the ground truth')
  ap.add_argument('--gt_crop', default=None, help='a Tanks and Temples crop file (JSON: bounding_polygon, orthogonal_axis, axis_min, axis_max)')
  ap.add_argument('--icp', choices=('none', 'point', 'plane'), default='none', help='refine the transform by ICP before scoring')
  ap.add_argument('--icp_max_dist', default=None, help='a[,b,c]: the correspondence distance of every ICP stage, coarse to fine')
  ap.add_argument('--icp_iters', type=int, default=30, help='updates an ICP stage at the most')
  ap.add_argument('--icp_scale', action='store_true', help='estimate a scale as well (--icp point only)')
  ap.add_argument('--icp_samples', type=int, default=200_000, help='surface samples of the mesh that are registered')
  ap.add_argument('--geometry_normals', action='store_true', help='add the normal consistency')
  args = ap.parse_args(argv)
  if (args.geometry_only or args.error_ply or args.gt_transform or args.gt_crop or args.icp != 'none' or args.geometry_normals) and not args.gt_mesh:
    raise SystemExit('eval_mesh.py: --geometry_only, --error_ply, --gt_transform, --gt_crop, --icp and --geometry_normals need --gt_mesh')
  if args.icp != 'none':
    try:
      args.icp_max_dist = [float(v) for v in (args.icp_max_dist or '').split(',')]
    except ValueError:
      raise SystemExit('eval_mesh.py: --icp needs --icp_max_dist a[,b,c], positive distances') from None
    if args.icp == 'plane' and args.icp_scale:
      raise SystemExit('eval_mesh.py: --icp_scale needs --icp point')
  try:
    args.geometry_thresholds = None if args.geometry_thresholds is None else [float(v) for v in args.geometry_thresholds.split(',')]
    args.geometry_bbox = None if args.geometry_bbox is None else [float(v) for v in args.geometry_bbox.split(',')]
    if args.geometry_bbox is not None and len(args.geometry_bbox) != 6:
      raise ValueError
  except ValueError:
    raise SystemExit('eval_mesh.py: --geometry_thresholds takes numbers a,b,... and --geometry_bbox six numbers x0,y0,z0,x1,y1,z1') from None
  try:
    args.bg = [float(v) for v in args.bg.split(',')]
    if len(args.bg) != 3:
      raise ValueError
  except ValueError:
    raise SystemExit(f'eval_mesh.py: --bg must be three numbers r,g,b') from None
  if args.supersample < 1:
    raise SystemExit('eval_mesh.py: --supersample must be at least 1')
  return args


def load_mesh(path, device):
  """(mesh dict on the device, texture dict or None, colours or None) of a PLY file."""
  m = mesh.read_ply(path)
  dm = {k: torch.from_numpy(np.ascontiguousarray(m[k])).to(device) for k in ('vertices', 'normals', 'faces')}
  texture = colors = None
  if m.get('texcoord') is not None:
    if not m.get('texture_file'):
      raise SystemExit(f'eval_mesh.py: {path} has texture coordinates but no `comment TextureFile` line')
    from PIL import Image
    png = os.path.join(os.path.dirname(os.path.abspath(path)), m['texture_file'])
    pixels = np.ascontiguousarray(np.asarray(Image.open(png).convert('RGB'), dtype=np.uint8))
    texture = dict(texture=torch.from_numpy(pixels).to(device), uv=torch.from_numpy(np.ascontiguousarray(m['texcoord'])).to(device))
    if m.get('texture_sh') is not None:
      if m['texture_sh'].shape[:2] != pixels.shape[:2]:
        raise SystemExit(f'eval_mesh.py: {m["texture_sh_file"]} is {m["texture_sh"].shape[:2]} texels, the texture {pixels.shape[:2]}')
      texture['sh'] = torch.from_numpy(m['texture_sh']).to(device)      # float32: read_ply has converted it
  elif m.get('colors') is not None:
    colors = torch.from_numpy(np.ascontiguousarray(m['colors'])).to(device)
  return dm, texture, colors


def score_geometry(args, dm, out_dir):
  """--gt_mesh: the metrics of mesh.geometry_metrics, mesh_metric_geometry.txt, the stage times and, with --error_ply, the error mesh."""
  from multinerf_amd import vis
  gt = mesh.read_ply_geometry(args.gt_mesh)
  transform = None
  if args.gt_transform:
    transform = np.loadtxt(args.gt_transform, dtype=np.float64).reshape(-1)
    if transform.shape != (16,):
      raise SystemExit(f'eval_mesh.py: {args.gt_transform} must hold 16 numbers, holds {transform.shape[0]}')
    transform = transform.reshape(4, 4)
  print(f'{args.gt_mesh}: {len(gt["vertices"])} vertices, {len(gt["faces"])} faces' + ('' if len(gt['faces']) else ' (a point cloud)'))
  crop = mesh.CropVolume.from_json(args.gt_crop) if args.gt_crop else None
  if args.icp != 'none':
    torch.cuda.synchronize()
    t0 = time.time()
    reg = mesh.register(dm, gt, init=transform, max_dist=args.icp_max_dist, mode=args.icp, with_scale=args.icp_scale,
                        max_iters=args.icp_iters, n_samples=args.icp_samples, crop=crop)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    for stage, md in enumerate(args.icp_max_dist):
      h = [e for e in reg['history'] if e['stage'] == stage]
      print(f'ICP stage {stage} (max_dist {md:g}): {len(h) - 1} iterations, fitness {h[0]["fitness"]:.6f} -> {h[-1]["fitness"]:.6f}, '
            f'rmse {h[0]["inlier_rmse"]:.6g} -> {h[-1]["inlier_rmse"]:.6g}')
    print(f'ICP seconds: {seconds:.4f} ({reg["iterations"]} iterations, {args.icp})')
    transform = reg['transform']
    np.savetxt(os.path.join(out_dir, 'mesh_gt_transform_refined.txt'), transform, fmt='%.17g')
  extra = dict(crop=crop, normals=True) if args.geometry_normals else dict(crop=crop) if crop is not None else {}
  timings = {}
  metrics = mesh.geometry_metrics(dm, gt, n_samples=args.geometry_samples, thresholds=args.geometry_thresholds, max_dist=args.geometry_max_dist,
                                  transform=transform, bbox=args.geometry_bbox, timings=timings, **extra)
  for name, value in metrics.items():
    print(f'{name} = {value:.9g}')
  with open(os.path.join(out_dir, 'mesh_metric_geometry.txt'), 'w') as f:
    f.write(''.join(f'{name} {value:.9g}\n' for name, value in metrics.items()))
  print('Geometry seconds: ' + ', '.join(f'{k} {timings[k]:.4f}' for k in ('sample', 'grid', 'query')))
  if args.error_ply:
    verts = dm['vertices']
    if transform is not None:
      h = verts.double().cpu().numpy() @ transform[:3, :3].T + transform[:3, 3]
      w = verts.double().cpu().numpy() @ transform[3, :3] + transform[3, 3]
      verts = torch.from_numpy((h / w[:, None]).astype(np.float32)).to(verts.device)
    d = mesh.point_mesh_distance(verts, gt, max_dist=args.geometry_max_dist)['distance']
    top = max(float(k.split('@')[1]) for k in metrics if k.startswith('fscore@'))
    d = d.clamp(max=top)[None].contiguous()                  # (one image row; lo = 0 would mean `automatic` to visualize_cmap)
    rgb = vis.visualize_cmap(d, torch.ones_like(d), 'turbo', lo=float(np.finfo(np.float32).tiny), hi=top, matte_background=False)
    rgb8 = (rgb.reshape(-1, 3).clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    mesh.write_ply(args.error_ply, dict(vertices=dm['vertices'], normals=dm['normals'], faces=dm['faces'], colors=rgb8))
    print(f'wrote {args.error_ply}: vertex colours turbo over 0 .. {top:g}')


def main(argv=None):
  args = parse_args(sys.argv[1:] if argv is None else argv)
  dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
  torch.cuda.set_device(dev)
  out_dir = args.out_dir or os.path.join(os.path.dirname(os.path.abspath(args.mesh)), 'mesh_eval')
  if args.geometry_only:
    dm = load_mesh(args.mesh, dev)[0]
    print(f'{args.mesh}: {dm["vertices"].shape[0]} vertices, {dm["faces"].shape[0]} faces')
    os.makedirs(out_dir, exist_ok=True)
    score_geometry(args, dm, out_dir)
    return
  config = configs.load_preset(args.preset, args.gin_bindings) if args.preset else \
      configs.load_config(args.gin_configs, args.gin_bindings, save_config=False)
  near = float(config.near if args.near is None else args.near)
  dm, texture, colors = load_mesh(args.mesh, dev)
  source = 'texture' if texture is not None else 'vertex colours' if colors is not None else 'shaded normals'
  print(f'{args.mesh}: {dm["vertices"].shape[0]} vertices, {dm["faces"].shape[0]} faces, colour from {source}')
  if texture is not None and texture.get('sh') is not None:
    degree = {1: 0, 4: 1, 9: 2}[int(texture['sh'].shape[2])]
    print(f'view-dependent texture: spherical harmonics of degree {degree}, ' +
          ('ignored (--no_view_dependent): the plain texture is scored' if args.no_view_dependent else "shaded at every pixel's view direction"))
  dataset = datasets.load_dataset(args.split, config.data_dir, config, device=dev)
  camtype = 'pano' if getattr(dataset, '_render_spherical', False) else dataset.camtype
  pixtocams = mesh._host(dataset.pixtocams, np.float64)
  os.makedirs(out_dir, exist_ok=True)
  harness = image.MetricHarness()
  quant, crop = bool(config.eval_quantize_metrics), int(config.eval_crop_borders)
  to_u8 = image.quantize_u8 if quant else (lambda x: (x.clamp(0, 1).cpu().numpy() * 255 + 0.5).astype(np.uint8))
  n = min(dataset.size, config.eval_dataset_limit)
  psnrs, ssims, seconds = [], [], []
  from PIL import Image
  method = args.method
  if method == 'auto':
    method = 'raster' if mesh.camera_is_pinhole(dataset.distortion_params, dataset.pixtocam_ndc, camtype) else 'raycast'
  print(f'rendering method: {method}' + (' (chosen by the cameras)' if args.method == 'auto' else ''))
  score = not dataset.render_path
  if not score:
    print('a render path has no images: the views are rendered and written, not scored')
  for idx in range(n):
    ptc = pixtocams if pixtocams.ndim == 2 else pixtocams[idx]
    kw = dict(texture=texture, colors=colors, near=near, bg=args.bg, cull=args.cull, supersample=args.supersample,
              view_dependent=not args.no_view_dependent)
    if method == 'raster':
      proj = mesh.world_to_pixel(ptc, dataset.camtoworlds[idx], distortion_params=dataset.distortion_params, pixtocam_ndc=dataset.pixtocam_ndc,
                                 camtype=camtype)
    torch.cuda.synchronize()
    t0 = time.time()
    if method == 'raster':
      r = mesh.render_mesh(dm, None, None, dataset.height, dataset.width, proj=proj, **kw)
    else:
      r = mesh.render_mesh(dm, ptc, dataset.camtoworlds[idx], dataset.height, dataset.width, method='raycast',
                           distortion_params=dataset.distortion_params, pixtocam_ndc=dataset.pixtocam_ndc, camtype=camtype, **kw)
    torch.cuda.synchronize()
    seconds.append(time.time() - t0)
    if score:
      gt = torch.as_tensor(dataset.images[idx]).to(device=dev, dtype=torch.float32)[..., :3].contiguous()
      metric = harness(r['rgb'].contiguous(), gt, quantize=quant, crop=crop)
      psnrs.append(metric['psnr'])
      ssims.append(metric['ssim'])
      print(f'Mesh image {idx + 1}/{n}: {seconds[-1]:.4f}s, psnr {metric["psnr"]:.3f}, ssim {metric["ssim"]:.4f}', flush=True)
    else:
      print(f'Mesh image {idx + 1}/{n}: {seconds[-1]:.4f}s', flush=True)
    Image.fromarray(to_u8(r['rgb'])).save(os.path.join(out_dir, f'mesh_color_{idx:03d}.png'))
  files = [('mesh_render_times.txt', seconds)]
  if score:
    print(f'Average mesh psnr over {n} images: {np.mean(psnrs):.3f}, ssim {np.mean(ssims):.4f}')
    files = [('mesh_metric_psnr.txt', psnrs), ('mesh_metric_ssim.txt', ssims)] + files
  for name, values in files:
    with open(os.path.join(out_dir, name), 'w') as f:
      f.write(' '.join(str(v) for v in values))
  if args.gt_mesh:
    score_geometry(args, dm, out_dir)


if __name__ == '__main__':
  main()
