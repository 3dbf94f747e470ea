"""Times of one ICP iteration of mesh.register (csrc/meshreg.hip) on the device, for profiles/mesh_registration.md.

    python tools/mesh_reg_probe.py [--resolution 236] [--samples 200000] [--iters 10]

Two marching-tetrahedra spheres as in profiles/mesh_geometry.md (A, radius 0.6, the source; B, radius 0.6 too, about 10^6 faces, the
target), A moved by a rotation of 2 degrees and a translation of 0.01.  mesh.register runs `iters` updates (rel_tol = 0) in mode
'plane' and 'point' against B's faces and against B's vertices as a point cloud with normals; its `timings` (each stage bracketed by
a device synchronisation, host clock, summed over the evaluations) are divided by the number of evaluations.  One untimed
registration first.  For the cloud, the same correspondence search on the host: scipy.spatial.cKDTree over the points, built once,
queried with the moved samples (float64, 16 workers).  Prints one JSON line.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sphere_mesh(resolution, radius, shift):
  from multinerf_amd import mesh, ops
  lo = (-0.75 + shift,) * 3
  shape, spacing = mesh.grid_shape(lo, tuple(v + 1.5 for v in lo), resolution)
  n = shape[0] * shape[1] * shape[2]
  field = torch.empty((n,), dtype=torch.float32, device='cuda')
  for start in range(0, n, 1 << 22):
    stop = min(start + (1 << 22), n)
    field[start:stop] = radius - mesh.grid_points(lo, spacing, shape, start, stop, 'cuda').norm(dim=-1)
  verts, normals, faces = ops.marching_tetrahedra(field.reshape(shape), 0., lo, spacing)
  return dict(vertices=verts, normals=normals, faces=faces)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--resolution', type=int, default=236)
  ap.add_argument('--samples', type=int, default=200_000)
  ap.add_argument('--iters', type=int, default=10)
  args = ap.parse_args()
  from multinerf_amd import mesh
  a, b = sphere_mesh(args.resolution, 0.6, 0.), sphere_mesh(args.resolution, 0.6, 0.0011)
  P = np.eye(4)
  P[:3, :3] = mesh._rodrigues(np.deg2rad(2.) * np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]))
  P[:3, 3] = [0.01, -0.006, 0.008]
  out = dict(faces_a=int(a['faces'].shape[0]), faces_b=int(b['faces'].shape[0]), points_b=int(b['vertices'].shape[0]), samples=args.samples,
             iters=args.iters)
  targets = {'mesh': dict(vertices=b['vertices'], faces=b['faces']), 'cloud': dict(vertices=b['vertices'], normals=b['normals'])}
  for tname, target in targets.items():
    for mode in ('plane', 'point'):
      kw = dict(init=P, max_dist=0.05, mode=mode, max_iters=args.iters, rel_tol=0., n_samples=args.samples)
      mesh.register(a, target, **kw)
      timings = {}
      torch.cuda.synchronize()
      t0 = time.time()
      reg = mesh.register(a, target, timings=timings, **kw)
      torch.cuda.synchronize()
      whole = time.time() - t0
      evals = len(reg['history'])
      out[f'{tname}_{mode}'] = dict(ms_per_iteration={k: 1e3 * v / evals for k, v in timings.items()}, evaluations=evals, whole_ms=1e3 * whole,
                                    fitness=reg['fitness'], rmse_first=reg['history'][0]['inlier_rmse'], rmse_last=reg['inlier_rmse'])
  # the host yardstick for the cloud: the same search with cKDTree
  from scipy.spatial import cKDTree
  pts = b['vertices'].double().cpu().numpy()
  src = mesh.sample_surface(a, args.samples)['points'].double().cpu().numpy() @ P[:3, :3].T + P[:3, 3]
  t0 = time.time()
  tree = cKDTree(pts)
  build = time.time() - t0
  qs = []
  for _ in range(5):
    t0 = time.time()
    d, idx = tree.query(src, distance_upper_bound=0.05, workers=16)
    qs.append(time.time() - t0)
  x = pts[np.minimum(idx, len(pts) - 1)]
  t0 = time.time()
  keep = np.isfinite(d)
  H = (src[keep] - src[keep].mean(0)).T @ (x[keep] - x[keep].mean(0))
  np.linalg.svd(H)
  solve = time.time() - t0
  out['ckdtree'] = dict(build_ms=1e3 * build, query_ms=1e3 * float(np.median(qs)), sums_and_svd_ms=1e3 * solve, found=int(keep.sum()))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
