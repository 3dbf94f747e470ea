"""Time the marching-tetrahedra passes and the grid query of a mesh extraction (profiles/mesh_extract.md).

    python tools/mesh_probe.py [--reps 9] [--sizes 256,512]       # the three passes of csrc/mesh.hip, HIP events
    python tools/mesh_probe.py --query [--points 4194304]         # Model.query_density, the 360 preset at full width

Isosurface part: the analytic sphere f = 0.6 - |x| on [-1, 1]^3 at n^3 points, level 0.  Each pass (mnr_mt_classify,
mnr_mt_emit_vertices, mnr_mt_emit_faces) is timed on its own: median HIP-event time over `reps` after two untimed calls,
next to a device-to-device copy in the same process; the clocks rocm-smi reports while the three passes run in a loop are noted.  "bytes that must move" per pass, from the shapes:
  classify       4 n^3 (field) + n^3 (mask)
  emit vertices  n^3 (mask) + 4 n^3 (base) + 24 V (positions, normals)
  emit faces     n^3 (mask) + 12 T (faces)
(what the passes read around the surface -- field, gradients, base of neighbours -- is O(n^2) and left out).  The whole
ops.marching_tetrahedra call (with its allocation, scan and read-back) is timed by the host clock around a synchronise.
Prints one JSON line.
"""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def clocks_under(fn, seconds=1.0):
  """`rocm-smi --showclocks --csv` sampled every 50 ms while fn() runs in a loop for `seconds`, and once idle: raw CSV lines."""
  cmd = ['rocm-smi', '--showclocks', '--csv']

  def sample():
    try:
      return subprocess.run(cmd, capture_output=True, text=True, timeout=5).stdout.strip().splitlines()
    except Exception as e:  # noqa: BLE001
      return [repr(e)]

  samples, run = [], [True]

  def poll():
    while run[0]:
      samples.append(sample()[-1:])
      time.sleep(0.05)

  th = threading.Thread(target=poll)
  th.start()
  t0 = time.time()
  while time.time() - t0 < seconds:
    for _ in range(20):
      fn()
    torch.cuda.synchronize()
  run[0] = False
  th.join()
  time.sleep(0.5)
  idle = sample()
  return dict(columns=idle[0] if idle else '?', idle=idle[-1] if idle else '?', under_load=[s[0] for s in samples[1:6] if s])


def isosurface_part(sizes, reps):
  from multinerf_amd import _lib as L, ops
  lib = ops.lib()
  out = dict(reps=reps)
  a = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
  b = torch.empty_like(a)
  copy_ms = timed(lambda: b.copy_(a), reps)
  out['copy_1GiB'] = dict(ms=copy_ms, gbps=2 * a.numel() / copy_ms / 1e6)
  copy_gbps = out['copy_1GiB']['gbps']
  del a, b
  for n in sizes:
    spacing = 2. / (n - 1)
    ax = -1. + spacing * torch.arange(n, dtype=torch.float32, device='cuda')
    field = (0.6 - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)).contiguous()
    origin = (-1., -1., -1.)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    verts, normals, faces = ops.marching_tetrahedra(field, 0., origin, spacing)
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t0
    whole = []
    for _ in range(reps):
      t0 = time.perf_counter()
      verts, normals, faces = ops.marching_tetrahedra(field, 0., origin, spacing)
      torch.cuda.synchronize()
      whole.append(time.perf_counter() - t0)
    V, T, N = int(verts.shape[0]), int(faces.shape[0]), n ** 3
    # the passes one by one, on buffers of their own (what ops.marching_tetrahedra does between them is the scan)
    nwg = int(lib.mnr_mt_workgroups(N))
    mask = torch.empty((N,), dtype=torch.uint8, device='cuda')
    counts = torch.empty((nwg, 2), dtype=torch.int32, device='cuda')
    base = torch.empty((N,), dtype=torch.int32, device='cuda')
    args = L.MtArgs()
    args.nx = args.ny = args.nz = n
    args.field, args.level, args.spacing = field.data_ptr(), 0., spacing
    args.origin[0], args.origin[1], args.origin[2] = origin
    args.mask, args.counts = mask.data_ptr(), counts.data_ptr()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.mnr_mt_classify(C.byref(args), stream()))
    scan = lambda: (lambda per: (torch.cumsum(per, 1, dtype=torch.int64) - per).t().contiguous())(counts.t().contiguous())
    offsets = scan()
    assert [int(v) for v in (offsets[-1] + counts[-1]).tolist()] == [V, T]
    v2, n2, f2 = torch.empty_like(verts), torch.empty_like(normals), torch.empty_like(faces)
    args.offsets, args.base = offsets.data_ptr(), base.data_ptr()
    args.verts, args.normals, args.n_verts, args.faces, args.n_faces = v2.data_ptr(), n2.data_ptr(), V, f2.data_ptr(), T
    passes = {}
    for name, fn, nbytes in (('classify', lib.mnr_mt_classify, 5 * N), ('emit_vertices', lib.mnr_mt_emit_vertices, 5 * N + 24 * V),
                             ('emit_faces', lib.mnr_mt_emit_faces, N + 12 * T)):
      ms = timed(lambda: L.check(fn(C.byref(args), stream())), reps)
      passes[name] = dict(ms=ms, bytes=nbytes, gbps=nbytes / ms / 1e6, of_copy=nbytes / ms / 1e6 / copy_gbps, of_5tbps=nbytes / ms / 1e6 / 5000.)
    assert torch.equal(v2, verts) and torch.equal(n2, normals) and torch.equal(f2, faces)
    three = lambda: [L.check(f(C.byref(args), stream())) for f in (lib.mnr_mt_classify, lib.mnr_mt_emit_vertices, lib.mnr_mt_emit_faces)]
    clocks = clocks_under(three)
    scan_ms = timed(scan, reps)
    out[f'sphere_{n}'] = dict(points=N, V=V, T=T, workgroups=nwg, passes=passes, clocks=clocks, scan_ms=scan_ms, whole_call_ms_median=1e3 * float(np.median(whole)),
                              whole_call_ms_first=1e3 * first_s)
    del field, mask, counts, base, verts, normals, faces, v2, n2, f2, offsets
    torch.cuda.empty_cache()
  return out


def query_part(points, chunk, reps):
  """Grid-query rate of the 360 preset (configs/360.gin) at full width: points per second of Model.query_density, chunk by chunk."""
  from multinerf_amd import configs, mesh, models
  config = configs.load_preset('360', [])
  model, _ = models.construct_model(0, None, config, device='cuda')
  n = round(points ** (1 / 3))
  fn = lambda x, s: model.query_density(x[None], s)[0]
  run = lambda: mesh.density_grid(fn, (-1., -1., -1.), (1., 1., 1.), n, std=0.5, chunk=chunk)
  run()
  torch.cuda.synchronize()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
  s = float(np.median(ts))
  return dict(config='360.gin', points=n ** 3, chunk=chunk, seconds_median=s, points_per_s=n ** 3 / s,
              peak_memory_gib=torch.cuda.max_memory_allocated() / 2 ** 30)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--sizes', default='256,512')
  ap.add_argument('--query', action='store_true')
  ap.add_argument('--points', type=int, default=1 << 22)
  ap.add_argument('--chunk', type=int, default=None)
  args = ap.parse_args()
  if args.query:
    from multinerf_amd import mesh
    print(json.dumps(query_part(args.points, args.chunk or mesh.DEFAULT_CHUNK, min(args.reps, 3))))
  else:
    print(json.dumps(isosurface_part([int(v) for v in args.sizes.split(',')], args.reps)))


if __name__ == '__main__':
  main()
