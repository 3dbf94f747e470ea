"""Time the mesh rasteriser (profiles/mesh_render.md).

    python tools/raster_probe.py [--reps 9] [--resolution 320] [--sizes 800,1600] [--thresholds 0,16,64,256,1024,4096,1048576] [--model]

A marching-tetrahedra sphere (radius 0.6, `--resolution` grid points a side: about 1 M faces at 320) and its `mesh.simplify`-d
version (cell of 4 spacings) are rendered at `--sizes` from outside (distance 2.5, the sphere fills most of the frame) and from
inside (every face behind or across the camera plane has the whole image as its box): median HIP-event time of
ops.raster_visibility (fill + small-face + large-face kernels) and of ops.raster_shade (vertex colours) over `reps` after two
untimed calls.  The threshold A/B times visibility alone for every `--thresholds` value on the outside views in one process.
--model adds the 360 preset's own render rate on the same device (one 16384-ray chunk, as bench.py times it) and what a frame
costs at that rate.  Prints one JSON line.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS = 0.6


def timed(fn, reps):
  """Median HIP-event time in ms of fn(), after two untimed calls."""
  fn()
  fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
  return float(np.median(ts))


def look_at(eye, target):
  eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
  fwd = (target - eye) / np.linalg.norm(target - eye)
  right = np.cross(fwd, [0., 0., 1.])
  right /= np.linalg.norm(right)
  return np.stack([right, np.cross(right, fwd), -fwd, eye], -1)


def sphere_mesh(resolution):
  from multinerf_amd import mesh, ops
  shape, spacing = mesh.grid_shape((-1.,) * 3, (1.,) * 3, resolution)
  n = shape[0] * shape[1] * shape[2]
  field = torch.empty((n,), dtype=torch.float32, device='cuda')
  for start in range(0, n, 1 << 22):
    stop = min(start + (1 << 22), n)
    field[start:stop] = RADIUS - mesh.grid_points((-1.,) * 3, spacing, shape, start, stop, 'cuda').norm(dim=-1)
  verts, normals, faces = ops.marching_tetrahedra(field.reshape(shape), 0., (-1.,) * 3, spacing)
  colors = (255 * (0.5 + 0.5 * normals)).to(torch.uint8).contiguous()
  return dict(vertices=verts, normals=normals, faces=faces, colors=colors), spacing


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--resolution', type=int, default=320)
  ap.add_argument('--sizes', default='800,1600')
  ap.add_argument('--thresholds', default='0,16,64,256,1024,4096,1048576')
  ap.add_argument('--model', action='store_true')
  args = ap.parse_args()
  from multinerf_amd import mesh, ops
  full, spacing = sphere_mesh(args.resolution)
  simple = mesh.simplify(full, 4. * spacing)
  out = dict(reps=args.reps, default_threshold=ops.RASTER_THRESHOLD, device=torch.cuda.get_device_name(0))
  views = dict(outside=((2.0, 1.2, 0.8), (0., 0., 0.), 2.2), inside=((0.1, -0.05, 0.15), (1., 0.3, 0.2), 0.35))      # focal / width
  thresholds = [int(t) for t in args.thresholds.split(',')]
  for name, m in (('marching_tetrahedra', full), ('simplified', simple)):
    res = dict(vertices=int(m['vertices'].shape[0]), faces=int(m['faces'].shape[0]))
    for size in (int(s) for s in args.sizes.split(',')):
      for view, (eye, target, f) in views.items():
        K = np.array([[f * size, 0., size / 2.], [0., f * size, size / 2.], [0., 0., 1.]])
        P = mesh.world_to_pixel(np.linalg.inv(K), look_at(eye, target))
        vis = ops.raster_visibility(m, P, size, size, 1e-3, check_faces=False)
        shaded = ops.raster_shade(m, P, vis, 1e-3, colors=m['colors'])
        key = f'{view}_{size}'
        res[key] = dict(covered=float((shaded['acc'] > 0).float().mean()),
                        visibility_ms=timed(lambda: ops.raster_visibility(m, P, size, size, 1e-3, check_faces=False), args.reps),
                        shade_ms=timed(lambda: ops.raster_shade(m, P, vis, 1e-3, colors=m['colors']), args.reps))
        if view == 'outside':
          ab = {}
          for t in thresholds:
            ab[str(t)] = timed(lambda: ops.raster_visibility(m, P, size, size, 1e-3, threshold=t, check_faces=False), args.reps)
            assert torch.equal(ops.raster_visibility(m, P, size, size, 1e-3, threshold=t, check_faces=False), vis)
          res[key]['visibility_ms_by_threshold'] = ab
    out[name] = res
  if args.model:
    from multinerf_amd import configs, synthetic, train_utils
    cfg = configs.load_preset('360')
    model, state, render_eval_pfn, _, _ = train_utils.setup_model(cfg, 0, device=torch.device('cuda', 0))
    rays = synthetic.synthetic_rays(16384, seed=20200823, near=cfg.near, far=cfg.far).map(lambda t: t.to('cuda')).rays
    ms = timed(lambda: render_eval_pfn(state.params, 1.0, None, rays), 5)
    out['model_360'] = dict(ms_per_16384_rays=ms, rays_per_s=16384 / ms * 1e3,
                            frame_ms={s: int(s) ** 2 / (16384 / ms) for s in args.sizes.split(',')})
  print(json.dumps(out))


if __name__ == '__main__':
  main()
