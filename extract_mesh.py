#!/usr/bin/env python
"""Mesh extraction script: restore the latest checkpoint and write the isosurface of the NeRF level's density inside a box
as a PLY file (binary_little_endian 1.0; positions, normals, optionally vertex colours, triangles).

The density is queried on a regular grid on the device (`Model.query_density`, chunk by chunk), the surface is taken by
marching tetrahedra on the device (`ops.marching_tetrahedra`, csrc/mesh.hip) and coloured by the NeRF MLP seen head-on
(`multinerf_amd.mesh`).  --bbox is in world coordinates; the default is the linear region of the contraction, larger boxes
are legal (the query warps like any other).  --density_threshold is scene-dependent: a decision, not a derived number.

--method tsdf meshes what the model RENDERS instead: every --tsdf_stride-th camera of the --tsdf_split split is rendered as
render.py renders it, and the depth (--tsdf_depth), opacity and colour images are fused into a truncated signed distance
volume over the box (`mesh.tsdf_mesh`, csrc/tsdf.hip), whose zero set between observed voxels is the surface.  It has no level
to choose; rays with opacity below --acc_threshold carve free space; colours come from the renders.  --tsdf_trunc, the
truncation in grid spacings, is a decision: larger closes thin gaps and thickens thin structures.  Every camera model is fused:
an undistorted pinhole through its [3,4] matrix, lens distortion (COLMAP OPENCV), fisheye (OPENCV_FISHEYE) and the spherical
Config.render_camtype = 'pano' through the forward camera model (`mesh.camera_record`); the run prints which.  Only an NDC ray
space (forward_facing) is refused: the distance rendered there is not a world distance.

--min_component_faces / --keep_largest drop small connected components (`mesh.filter_components`: floaters are little closed
shells of their own) and --simplify F merges the vertices of every cube of F grid spacings into one, placed by the quadric
error of the faces around it (`mesh.simplify`, csrc/meshclean.hip); components first, then simplification, with either method.
With all three at their defaults nothing of this runs and the file is the one written before.

--texture C bakes a texture atlas after the clean-up (`mesh.bake_texture`, csrc/atlas.hip): every face gets a chart of C texels a
side, every texel is coloured by the NeRF MLP at the Gaussian of its own footprint (--texture_filter texels wide), and the file
carries per-face texture coordinates next to <out>.png; --out x.obj writes OBJ + MTL + PNG instead of PLY.  So
--simplify 4 --texture 8 gives a mesh about 16 times lighter with more colour samples per area than the vertex-coloured original.
With --method tsdf the texture comes from the MLP as well; the vertex colours stay the fused ones.  An atlas with a side above
--texture_max_side is refused before anything is baked.

--texture_sh L (0, 1 or 2; needs --texture) additionally fits, per texel, spherical harmonics of degree L to the MLP's colour over
the view directions the texel can be seen from (--texture_sh_dirs 2: 42 directions, 3: 92; --texture_sh_lambda: the ridge;
`mesh.bake_texture(sh_degree=)`, csrc/shtex.hip) and writes them as <out>_sh.npy (--texture_sh_dtype float16 or float32), named in
the PLY header; eval_mesh.py and mesh.render_mesh then shade every pixel at its own view direction.  A model whose MLP reads no
view direction is refused: nothing would change.

  python extract_mesh.py --gin_configs configs/360.gin --gin_bindings "Config.checkpoint_dir = '...'" \
      --resolution 512 --density_threshold 10 --out garden.ply
  python extract_mesh.py --gin_configs configs/360.gin --gin_bindings "Config.checkpoint_dir = '...'" \
      --gin_bindings "Config.data_dir = '...'" --method tsdf --resolution 512 --out garden_tsdf.ply
"""

import argparse
import math
import os
import sys
import time

import torch

from multinerf_amd import _lib, checkpoints, configs, mesh, ops, train_utils


def parse_args(argv):
  """(args, box) of the command line `argv`; box = [x0, y0, z0, x1, y1, z1]."""
  ap = argparse.ArgumentParser()
  ap.add_argument('--gin_configs', action='append', default=[])
  ap.add_argument('--gin_bindings', action='append', default=[])
  ap.add_argument('--preset', default=None)
  ap.add_argument('--resolution', type=int, default=256, help='grid points along the longest side of the box')
  ap.add_argument('--bbox', default='-1,-1,-1,1,1,1', help='x0,y0,z0,x1,y1,z1 in world coordinates')
  ap.add_argument('--density_threshold', type=float, default=10.0, help='the isosurface level (scene-dependent)')
  ap.add_argument('--std', type=float, default=0.5, help='standard deviation of the query Gaussians in grid spacings (0: point samples)')
  ap.add_argument('--chunk', type=int, default=mesh.DEFAULT_CHUNK, help='points per MLP call')
  ap.add_argument('--no_colors', action='store_true')
  ap.add_argument('--out', default=None, help='default: <checkpoint_dir>/mesh/mesh_step_<step>.ply')
  ap.add_argument('--method', choices=('density', 'tsdf'), default='density',
                  help='density: the isosurface of the density; tsdf: fuse rendered depth into a truncated signed distance volume')
  ap.add_argument('--tsdf_trunc', type=float, default=3.0,
                  help='truncation distance in grid spacings (a decision: larger closes thin gaps and thickens thin structures)')
  ap.add_argument('--tsdf_split', choices=('train', 'test'), default='train', help='the cameras to render')
  ap.add_argument('--tsdf_stride', type=int, default=1, help='render every n-th camera')
  ap.add_argument('--tsdf_depth', choices=('distance_median', 'distance_mean'), default='distance_median')
  ap.add_argument('--acc_threshold', type=float, default=0.5, help='rays with less opacity are empty: they carve free space')
  ap.add_argument('--min_component_faces', type=int, default=0, help='drop connected components with fewer faces (0: keep all)')
  ap.add_argument('--keep_largest', type=int, default=0, help='keep only this many components with the most faces (0: keep all)')
  ap.add_argument('--simplify', type=float, default=0., help='vertex clustering with a cell of this many grid spacings (0: off)')
  ap.add_argument('--texture', type=int, default=0, help='bake a texture atlas with face charts of this many texels a side (0: off; else >= 3)')
  ap.add_argument('--texture_filter', type=float, default=1.0, help="width of a texel's query Gaussian in texels (0: point samples)")
  ap.add_argument('--texture_max_side', type=int, default=16384,
                  help='refuse an atlas with a longer side (a decision: 16384 is the common hardware texture limit)')
  ap.add_argument('--texture_sh', type=int, default=None, choices=tuple(range(_lib.SHTEX_MAX_DEGREE + 1)),
                  help='also fit per-texel spherical harmonics of this degree over the view directions (default: off; needs --texture)')
  ap.add_argument('--texture_sh_dirs', type=int, default=2, choices=(2, 3), help='icosahedron tesselation of the fitted directions: 42 or 92')
  ap.add_argument('--texture_sh_lambda', type=float, default=1e-3, help='ridge of the fit on all coefficients but the constant (a decision)')
  ap.add_argument('--texture_sh_dtype', choices=mesh.SH_DTYPES, default='float16', help='storage of <out>_sh.npy')
  # `--bbox -1,-1,-1,1,1,1`: argparse takes a value that starts with '-' and is no plain number for an option; hand it over as --bbox=...
  argv = list(argv)
  for i in range(len(argv) - 1):
    if argv[i] == '--bbox':
      argv[i:i + 2] = ['--bbox=' + argv[i + 1]]
      break
  args = ap.parse_args(argv)
  try:
    box = [float(v) for v in args.bbox.split(',')]
    if len(box) != 6:
      raise ValueError
  except ValueError:
    raise SystemExit(f'extract_mesh.py: --bbox {args.bbox!r} must be six numbers x0,y0,z0,x1,y1,z1') from None
  if args.min_component_faces < 0 or args.keep_largest < 0 or not (0. <= args.simplify < float('inf')):
    raise SystemExit('extract_mesh.py: --min_component_faces, --keep_largest and --simplify must not be negative')
  if args.texture != 0 and args.texture < _lib.ATLAS_MIN_CELL:
    raise SystemExit(f'extract_mesh.py: --texture must be 0 (off) or at least {_lib.ATLAS_MIN_CELL}')
  if not (0. <= args.texture_filter < float('inf')) or args.texture_max_side < 1:
    raise SystemExit('extract_mesh.py: --texture_filter must be finite and not negative, --texture_max_side positive')
  if args.texture_sh is not None and args.texture == 0:
    raise SystemExit('extract_mesh.py: --texture_sh needs --texture: the harmonics live in the texture atlas')
  if not (0. <= args.texture_sh_lambda < float('inf')):
    raise SystemExit('extract_mesh.py: --texture_sh_lambda must be finite and not negative')
  return args, box


def _format_stats(stats):
  return ', '.join(f'{k} {v:.6g}' if isinstance(v, float) else f'{k} {v}' for k, v in stats.items())


def _clean_up_seconds(args, t_comp, t_simp):
  if args.min_component_faces == 0 and args.keep_largest == 0 and args.simplify == 0.:
    return ''
  return f', components {t_comp:.3f}, simplify {t_simp:.3f}'


def clean_up(args, result, spacing, timed):
  """(the mesh after --min_component_faces / --keep_largest and --simplify, seconds of the components step, seconds of the
  simplification); the mesh itself and (0, 0) when all three are at their defaults.  Prints the statistics before and after."""
  if args.min_component_faces == 0 and args.keep_largest == 0 and args.simplify == 0.:
    return result, 0., 0.
  report = lambda label, m: print(f'{label}: mesh_stats: {_format_stats(mesh.mesh_stats(m["vertices"], m["faces"]))}; '
                                  f'components {mesh.component_stats(m)["count"]}')
  report('before clean-up', result)
  t_comp = t_simp = 0.
  if args.min_component_faces > 0 or args.keep_largest > 0:
    result, t_comp = timed(lambda: mesh.filter_components(result, min_faces=args.min_component_faces, keep_largest=args.keep_largest))
  if args.simplify > 0.:
    result, t_simp = timed(lambda: mesh.simplify(result, args.simplify * spacing))
  report('after clean-up', result)
  return result, t_comp, t_simp


def bake_and_write(args, model, result, out, timed):
  """Write `result` to `out` (OBJ for an .obj name, else PLY), with a texture atlas baked from the model's NeRF MLP when --texture is
  set; returns (seconds of the bake, seconds of the file write, of the bake's seconds those of the SH fit).  An atlas beyond
  --texture_max_side stops the script before the bake and names the --simplify factor that would fit."""
  texture, t_bake, seconds = None, 0., {}
  n_faces = int(result['faces'].shape[0])
  if args.texture > 0 and n_faces > 0:
    layout = ops.atlas_layout(n_faces, args.texture)
    side = max(layout['W'], layout['H'])
    if side > args.texture_max_side:
      # the face count falls with the square of the clustering cell, the atlas side with the root of the face count
      factor = math.ceil((args.simplify if args.simplify > 0. else 1.) * side / args.texture_max_side * 10.) / 10.
      raise SystemExit(f'extract_mesh.py: the atlas of {n_faces} faces at --texture {args.texture} is {layout["W"]} x {layout["H"]} texels, beyond '
                       f'--texture_max_side {args.texture_max_side}; about --simplify {factor:.1f} would fit')
    print(f'texture: {layout["W"]} x {layout["H"]}, {layout["n_samples"]} samples, cell {args.texture}')
    sh = {} if args.texture_sh is None else dict(sh_degree=args.texture_sh, sh_dirs=args.texture_sh_dirs, sh_lambda=args.texture_sh_lambda,
                                                 timings=seconds)
    texture, t_bake = timed(lambda: mesh.bake_texture(result, model=model, cell=args.texture, filter=args.texture_filter, chunk=args.chunk, **sh))
    if args.texture_sh is not None:
      print(f'texture sh: degree {args.texture_sh}, {int(texture["sh_dirs"].shape[0])} directions, {texture["sh_queries"]} colour queries')
  elif args.texture > 0:
    print('texture: the mesh has no faces, nothing to bake')
  os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
  if out.lower().endswith('.obj'):
    if texture is None:
      raise SystemExit('extract_mesh.py: --out x.obj needs --texture (and a mesh with faces): the OBJ writer writes textured meshes')
    _, t_write = timed(lambda: mesh.write_obj(out, result, texture, sh_dtype=args.texture_sh_dtype))
  else:
    _, t_write = timed(lambda: mesh.write_ply(out, result, texture=texture, sh_dtype=args.texture_sh_dtype))
  return t_bake, t_write, seconds.get('sh', 0.)


def _texture_seconds(args, t_bake, t_sh=0.):
  if args.texture_sh is not None:
    return f', texture bake {t_bake:.3f} (sh {t_sh:.3f})'
  return f', texture bake {t_bake:.3f}' if args.texture > 0 else ''


def main():
  args, box = parse_args(sys.argv[1:])
  dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
  torch.cuda.set_device(dev)
  config = configs.load_preset(args.preset, args.gin_bindings) if args.preset else \
      configs.load_config(args.gin_configs, args.gin_bindings, save_config=False)
  model, state, _, _, _ = train_utils.setup_model(config, 20200823, dataset=None, device=dev)
  if args.texture_sh is not None and not model.nerf_plan.use_viewdirs:
    raise SystemExit("extract_mesh.py: --texture_sh: this model's MLP reads no view direction, nothing would change")
  if not config.checkpoint_dir or checkpoints.latest_checkpoint(config.checkpoint_dir) is None:
    raise SystemExit(f'extract_mesh.py: no checkpoint in Config.checkpoint_dir = {config.checkpoint_dir!r}')
  state = checkpoints.restore_checkpoint(config.checkpoint_dir, model, state)
  step = int(state.step)
  print(f'Extracting a mesh from the checkpoint at step {step}.')
  out = args.out or os.path.join(config.checkpoint_dir, 'mesh', f'mesh_step_{step}.ply')

  def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    r = fn()
    torch.cuda.synchronize()
    return r, time.time() - t0

  if args.method == 'tsdf':
    return main_tsdf(args, box, config, model, state, out, timed)

  (field, origin, spacing), t_grid = timed(lambda: mesh.density_grid(
      lambda x, s: model.query_density(x[None], s)[0], box[:3], box[3:], args.resolution, std=args.std, chunk=args.chunk, device=dev))
  print(f'grid {tuple(field.shape)}, spacing {spacing:.6g}, density min {float(field.min()):.4g} max {float(field.max()):.4g}')
  (verts, normals, faces), t_iso = timed(lambda: ops.marching_tetrahedra(field, args.density_threshold, origin, spacing))
  colors, t_col = None, 0.
  if not args.no_colors:
    colors, t_col = timed(lambda: mesh.vertex_colors(model, verts, normals, args.std * spacing, args.chunk))
  result = dict(vertices=verts, normals=normals, faces=faces, colors=colors)
  result, t_comp, t_simp = clean_up(args, result, spacing, timed)
  verts, faces = result['vertices'], result['faces']
  t_bake, t_write, t_sh = bake_and_write(args, model, result, out, timed)
  stats = mesh.mesh_stats(verts, faces)
  print('mesh_stats: ' + _format_stats(stats))
  print(f'seconds: grid query {t_grid:.3f} ({field.numel() / max(t_grid, 1e-9):.4g} points/s), isosurface {t_iso:.3f}, '
        f'colour query {t_col:.3f}, file write {t_write:.3f}' + _clean_up_seconds(args, t_comp, t_simp) + _texture_seconds(args, t_bake, t_sh))
  print(f'wrote {out}')


def main_tsdf(args, box, config, model, state, out, timed):
  from multinerf_amd import datasets
  dataset = datasets.load_dataset(args.tsdf_split, config.data_dir, config, device=model.device)
  seconds = {}
  try:
    result, volume = mesh.tsdf_mesh(model, state.params, dataset, config, box[:3], box[3:], args.resolution, trunc_voxels=args.tsdf_trunc,
                                    depth_key=args.tsdf_depth, acc_threshold=args.acc_threshold, frame_stride=args.tsdf_stride,
                                    colors=not args.no_colors, timings=seconds)
  except ValueError as e:                                  # (a camera model that cannot be fused: NDC; tsdf_mesh says why)
    raise SystemExit(f'extract_mesh.py: --method tsdf: {e}') from None
  frames = len(range(0, dataset.size, args.tsdf_stride))
  print(f'grid {tuple(volume.shape)}, spacing {volume.spacing:.6g}, truncation {volume.trunc:.6g}, {frames} frames of '
        f'{dataset.height} x {dataset.width} ({args.tsdf_split} split, {args.tsdf_depth})')
  print(f'projection: {volume.projection}')
  kept_faces = int(result['faces'].shape[0])
  result, t_comp, t_simp = clean_up(args, result, volume.spacing, timed)
  t_bake, t_write, t_sh = bake_and_write(args, model, result, out, timed)
  stats = mesh.mesh_stats(result['vertices'], result['faces'])
  print('mesh_stats: ' + _format_stats(stats))
  unseen, total = int((volume.weight == 0).sum()), volume.weight.numel()
  print(f'never observed: {unseen} of {total} voxels ({unseen / total:.2%})')
  before = int(ops.marching_tetrahedra(volume.field()[0], 0., volume.origin, volume.spacing)[2].shape[0])
  print(f'faces: {before} before the validity filter, {kept_faces} after')
  print(f'seconds: render {seconds["render"]:.3f}, fusion {seconds["fusion"]:.3f}, isosurface {seconds["isosurface"]:.3f}, '
        f'file write {t_write:.3f}' + _clean_up_seconds(args, t_comp, t_simp) + _texture_seconds(args, t_bake, t_sh))
  print(f'wrote {out}')


if __name__ == '__main__':
  main()
