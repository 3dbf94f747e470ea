"""Time the mesh ray caster next to the rasteriser (profiles/mesh_raycast.md).

    python tools/raycast_probe.py [--reps 9] [--resolutions 33,320] [--size 800]

Marching-tetrahedra spheres (radius 0.6; `--resolutions` grid points a side: about 10^4 faces at 33, the spacing of the tests'
10,364-face sphere, and about 10^6 at 320) are rendered at `--size` x `--size` from outside (distance 2.5, the sphere fills most of
the frame) and from inside, pinhole: median HIP-event time over `reps`, after two untimed calls, of
  ops.mesh_raycast with the 8 x 8 tile order, with row-major order and with its own entry-cell sort (torch sort included),
  ops.raycast_shade (vertex colours), and
  ops.raster_visibility + ops.raster_shade on the same view,
and once each: the grid build, the ray construction, the tile order.  A fisheye view of the same size goes through the ray caster
only.  Prints one JSON line.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from raster_probe import look_at, sphere_mesh, timed  # noqa: E402


def wall(fn):
  torch.cuda.synchronize()
  t0 = time.time()
  out = fn()
  torch.cuda.synchronize()
  return out, 1e3 * (time.time() - t0)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--resolutions', default='33,320')
  ap.add_argument('--size', type=int, default=800)
  args = ap.parse_args()
  from multinerf_amd import camera_utils, mesh, ops
  S = args.size
  out = dict(reps=args.reps, size=S, device=torch.cuda.get_device_name(0) if os.path.exists('/dev/kfd') else 'none')
  views = dict(outside=((2.0, 1.2, 0.8), (0., 0., 0.), 2.2), inside=((0.1, -0.05, 0.15), (1., 0.3, 0.2), 0.35))      # focal / width
  ys, xs = torch.meshgrid(torch.arange(S, dtype=torch.int32, device='cuda'), torch.arange(S, dtype=torch.int32, device='cuda'), indexing='ij')
  tile, out['tile_order_ms'] = wall(lambda: ops.pixel_tile_order(S, S, 'cuda'))
  tile, out['tile_order_ms'] = wall(lambda: ops.pixel_tile_order(S, S, 'cuda'))
  rows = torch.arange(S * S, device='cuda')
  for resolution in (int(v) for v in args.resolutions.split(',')):
    m = sphere_mesh(resolution)[0]
    v, f = m['vertices'], m['faces']
    grid, grid_ms = wall(lambda: ops.mesh_grid_build(v, f))
    grid, grid_ms = wall(lambda: ops.mesh_grid_build(v, f))
    res = dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), grid_build_ms=grid_ms, grid_dims=grid['dims'], grid_pairs=grid['pairs'])
    for view, (eye, target, fw) in views.items():
      ptc = np.linalg.inv(np.array([[fw * S, 0, S / 2.], [0, fw * S, S / 2.], [0, 0, 1.]]))
      c2w = look_at(eye, target)
      P = mesh.world_to_pixel(ptc, c2w)
      for cam in ('pinhole', 'fisheye'):
        camtype = camera_utils.ProjectionType.FISHEYE if cam == 'fisheye' else camera_utils.ProjectionType.PERSPECTIVE
        rays = lambda: camera_utils.pixels_to_rays(xs, ys, torch.as_tensor(ptc, dtype=torch.float32).cuda(), torch.as_tensor(c2w, dtype=torch.float32).cuda(),
                                                   camtype=camtype)[:2]
        (o, d), rays_ms = wall(rays)
        (o, d), rays_ms = wall(rays)
        o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
        cast = lambda order: ops.mesh_raycast(o, d, v, f, t_min=0.05, grid=grid, order=order, check_faces=False)
        t, face, bary = cast(tile)
        r = dict(rays_ms=rays_ms, hit=int((face >= 0).sum()), raycast_tile_ms=timed(lambda: cast(tile), args.reps),
                 raycast_rowmajor_ms=timed(lambda: cast(rows), args.reps), raycast_entry_sort_ms=timed(lambda: cast(None), args.reps),
                 raycast_shade_ms=timed(lambda: ops.raycast_shade(m, face, bary, colors=m['colors']), args.reps))
        r['rays_per_s_tile'] = S * S / (1e-3 * r['raycast_tile_ms'])
        if cam == 'pinhole':
          vis = ops.raster_visibility(m, P, S, S, 0.05, check_faces=False)
          r['raster_visibility_ms'] = timed(lambda: ops.raster_visibility(m, P, S, S, 0.05, check_faces=False), args.reps)
          r['raster_shade_ms'] = timed(lambda: ops.raster_shade(m, P, vis, 0.05, colors=m['colors']), args.reps)
          rf = ops.raster_shade(m, P, vis, 0.05, colors=m['colors'])['face'].reshape(-1)
          r['faces_differ'] = int((rf != face).sum())
        res[f'{view}_{cam}'] = r
    out[f'resolution_{resolution}'] = res
  print(json.dumps(out))


if __name__ == '__main__':
  main()
