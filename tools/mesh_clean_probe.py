"""Time the mesh clean-up (profiles/mesh_clean.md).

    python tools/mesh_clean_probe.py [--reps 5] [--sizes 256,512] [--cells 2,4]

The analytic sphere of profiles/mesh_extract.md (f = 0.6 - |x| on n^3 points over [-1, 1]^3, level 0) is meshed by
ops.marching_tetrahedra, then: mesh.filter_components(min_faces=1) (the labelling, the counts and the compaction) and
mesh.simplify at every cell size (in grid spacings).  Each is the median host-clock time over `reps` calls that end in a device
synchronise, after two untimed calls; they contain their read-backs.  "kernels" is the HIP-event time spent inside the
csrc/meshclean.hip entries during one further call (the ops wrappers are bracketed with events for that call only); the rest
of a call is torch: sorts, unique, scans, compaction, read-backs.  Prints one JSON line.
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


def timed(fn, reps):
  fn()
  fn()
  ts = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ts))


def kernel_ms(fn, names):
  """{name: HIP-event ms inside ops.<name>} over one call of fn()."""
  from multinerf_amd import ops
  spent, saved = {n: 0. for n in names}, {n: getattr(ops, n) for n in names}

  def wrap(name):
    def call(*a, **k):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      r = saved[name](*a, **k)
      e1.record()
      torch.cuda.synchronize()
      spent[name] += e0.elapsed_time(e1)
      return r
    return call

  try:
    for n in names:
      setattr(ops, n, wrap(n))
    fn()
  finally:
    for n in names:
      setattr(ops, n, saved[n])
  return spent


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--sizes', default='256,512')
  ap.add_argument('--cells', default='2,4')
  args = ap.parse_args()
  from multinerf_amd import mesh, ops
  out = dict(reps=args.reps)
  for n in (int(v) for v in args.sizes.split(',')):
    field, origin, spacing = mesh.density_grid(lambda x, s: 0.6 - torch.sqrt((x * x).sum(-1)), (-1., -1., -1.), (1., 1., 1.), n, std=0.)
    iso_ms = timed(lambda: ops.marching_tetrahedra(field, 0., origin, spacing), args.reps)
    verts, normals, faces = ops.marching_tetrahedra(field, 0., origin, spacing)
    del field
    V, T = int(verts.shape[0]), int(faces.shape[0])
    colors = torch.randint(0, 256, (V, 3), dtype=torch.uint8, device='cuda', generator=torch.Generator('cuda').manual_seed(0))
    m = dict(vertices=verts, normals=normals, faces=faces, colors=colors)
    res = dict(V=V, T=T, isosurface_ms=iso_ms)
    labels, sweeps = ops.mesh_components(faces, V, return_sweeps=True)
    res['components'] = dict(ms=timed(lambda: mesh.filter_components(m, min_faces=1), args.reps),
                             labelling_ms=timed(lambda: ops.mesh_components(faces, V), args.reps), sweeps=sweeps,
                             count=int(torch.unique(labels).shape[0]),
                             kernels_ms=kernel_ms(lambda: mesh.filter_components(m, min_faces=1), ['mesh_components']))
    for c in (float(v) for v in args.cells.split(',')):
      call = lambda: mesh.simplify(m, c * spacing)
      s = call()
      V2, T2 = int(s['vertices'].shape[0]), int(s['faces'].shape[0])
      res[f'simplify_{c:g}'] = dict(ms=timed(call, args.reps), V_out=V2, T_out=T2, V_ratio=V2 / V, T_ratio=T2 / T,
                                    kernels_ms=kernel_ms(call, ['mesh_cluster_keys', 'mesh_cluster_faces', 'mesh_cluster_solve']),
                                    stats=mesh.mesh_stats(s['vertices'], s['faces']))
      del s
    out[f'sphere_{n}'] = res
    del m, verts, normals, faces, colors, labels
    torch.cuda.empty_cache()
  print(json.dumps(out))


if __name__ == '__main__':
  main()
