"""Time the texture atlas (profiles/texture_atlas.md).

    python tools/atlas_probe.py [--reps 9] [--grid 708] [--cell 8] [--bake_grid 708] [--chunk 262144] [--bake_reps 9]

Kernels.  A height field over a grid of `grid`^2 squares (2 grid^2 faces: 708 gives 1.0 M) is sampled at `cell` texels in ONE call of
ops.atlas_samples (all of its samples; no index read-back) and stored by one call of ops.atlas_store; each is the median HIP-event
time over `reps` calls after two untimed ones.  Bytes are the algorithm's: samples writes 76 B a sample (19 floats and the face) and
reads the mesh once; store reads 16 B a sample (rgb and face) and writes 4 B a texel (rgb8 and the mask).  The yardstick is a
device-to-device copy of the samples' output size in the same process (bytes = read + written).

End to end.  A height field of `bake_grid`^2 squares is baked from a model with random weights (the blender_256 preset at full width),
`mesh.bake_texture(model=...)` at `chunk` samples an MLP call, next to `mesh.vertex_colors` on as many points at the same chunk:
the same MLP call behind both.  Host clock around calls that end in a device synchronise, `bake_reps` of each, alternating; the
parts of a bake are the HIP-event times inside ops.atlas_samples / ops.atlas_store during one further bake.  Prints one JSON line.
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


def height_field(n, device='cuda'):
  """dict(vertices, normals, faces) of z = 0.2 sin(3 x) cos(2 y) over [-1, 1]^2 on (n + 1)^2 vertices, 2 n^2 faces in grid order."""
  t = torch.linspace(-1., 1., n + 1, device=device)
  x, y = torch.meshgrid(t, t, indexing='ij')
  z = 0.2 * torch.sin(3. * x) * torch.cos(2. * y)
  verts = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
  normals = torch.nn.functional.normalize(torch.stack([-0.6 * torch.cos(3. * x) * torch.cos(2. * y), 0.4 * torch.sin(3. * x) * torch.sin(2. * y),
                                                       torch.ones_like(x)], -1), dim=-1).reshape(-1, 3).contiguous()
  i, j = torch.meshgrid(torch.arange(n, device=device), torch.arange(n, device=device), indexing='ij')
  a = (i * (n + 1) + j).reshape(-1)
  lower, upper = torch.stack([a, a + n + 1, a + 1], -1), torch.stack([a + n + 2, a + 1, a + n + 1], -1)
  faces = torch.stack([lower, upper], 1).reshape(-1, 3).to(torch.int32).contiguous()
  return dict(vertices=verts, normals=normals, faces=faces)


def event_ms(fn, reps):
  fn()
  fn()
  ts = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
  return float(np.median(ts)), float(min(ts)), float(max(ts))


def host_s(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return time.perf_counter() - t0


def parts_ms(fn, names):
  """{name: HIP-event ms inside ops.<name>} over one call of fn() (the wrappers synchronise: not a timing of fn itself)."""
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
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--grid', type=int, default=708)
  ap.add_argument('--cell', type=int, default=8)
  ap.add_argument('--bake_grid', type=int, default=708, help='0: the kernels only')
  ap.add_argument('--bake_reps', type=int, default=9)
  ap.add_argument('--chunk', type=int, default=1 << 18)
  ap.add_argument('--preset', default='blender_256')
  args = ap.parse_args()
  from multinerf_amd import configs, mesh, models, ops
  out = dict(reps=args.reps, cell=args.cell, device=torch.cuda.get_device_name(0))

  # ---- the kernels on their own
  m = height_field(args.grid)
  T, V = int(m['faces'].shape[0]), int(m['vertices'].shape[0])
  lay = ops.atlas_layout(T, args.cell)
  n = lay['n_samples']
  sample = lambda: ops.atlas_samples(m, lay, 0, n, check_faces=False)
  ms, lo, hi = event_ms(sample, args.reps)
  written, read = 76 * n, 12 * T + 24 * V
  out['samples'] = dict(T=T, V=V, n_samples=n, W=lay['W'], H=lay['H'], ms=ms, ms_min=lo, ms_max=hi, bytes_written=written, bytes_read_once=read,
                        GBps=(written + read) / ms / 1e6)
  means, covs, normals, viewdirs, face = sample()
  src = torch.empty((19 * n,), dtype=torch.float32, device='cuda').normal_()
  dst = torch.empty_like(src)
  ms, lo, hi = event_ms(lambda: dst.copy_(src), args.reps)
  out['copy'] = dict(bytes=2 * src.numel() * 4, ms=ms, ms_min=lo, ms_max=hi, GBps=2 * src.numel() * 4 / ms / 1e6)
  del src, dst, covs, normals, viewdirs
  rgb = (0.5 + 0.5 * means).contiguous()
  del means
  atlas, mask = torch.zeros((lay['H'], lay['W'], 3), dtype=torch.uint8, device='cuda'), torch.zeros((lay['H'], lay['W']), dtype=torch.uint8, device='cuda')
  ms, lo, hi = event_ms(lambda: ops.atlas_store(m, lay, 0, rgb, face, atlas, mask, check_faces=False), args.reps)
  moved = 16 * n + 4 * int((face >= 0).sum())
  out['store'] = dict(ms=ms, ms_min=lo, ms_max=hi, bytes=moved, GBps=moved / ms / 1e6)
  ms, lo, hi = event_ms(lambda: ops.atlas_uvs(m, lay), args.reps)
  out['uvs'] = dict(ms=ms, ms_min=lo, ms_max=hi, bytes=24 * T, GBps=24 * T / ms / 1e6)
  del rgb, face, atlas, mask, m
  torch.cuda.empty_cache()

  if args.bake_grid <= 0:
    print(json.dumps(out))
    return

  # ---- end to end: the bake next to vertex_colors, the same MLP call behind both
  config = configs.load_preset(args.preset, ["Config.dataset_loader = 'procedural'"])
  model, _ = models.construct_model(20200823, None, config, device='cuda')
  m = height_field(args.bake_grid)
  lay = ops.atlas_layout(int(m['faces'].shape[0]), args.cell)
  n = lay['n_samples']
  gen = torch.Generator('cuda').manual_seed(0)
  points = torch.rand((n, 3), device='cuda', generator=gen) * 2. - 1.
  dirs = torch.nn.functional.normalize(torch.randn((n, 3), device='cuda', generator=gen), dim=-1)
  spacing = 2. / args.bake_grid
  bake = lambda: mesh.bake_texture(m, model=model, cell=args.cell, chunk=args.chunk)
  colors = lambda: mesh.vertex_colors(model, points, dirs, 0.5 * spacing / (args.cell - 2), args.chunk)
  bake()
  colors()
  tb, tc = [], []
  for _ in range(args.bake_reps):
    tb.append(host_s(bake))
    tc.append(host_s(colors))
  parts = parts_ms(bake, ['atlas_samples', 'atlas_store', 'atlas_uvs'])
  total = host_s(bake)
  rate = lambda ts: dict(s_median=float(np.median(ts)), s_min=min(ts), s_max=max(ts), samples_per_s=n / float(np.median(ts)),
                         samples_per_s_min=n / max(ts), samples_per_s_max=n / min(ts))
  out['bake'] = dict(T=int(m['faces'].shape[0]), n_samples=n, chunk=args.chunk, chunks=-(-n // args.chunk), W=lay['W'], H=lay['H'], **rate(tb),
                     parts_ms=parts, one_bake_ms=total * 1e3)
  out['vertex_colors'] = dict(n_points=n, chunk=args.chunk, **rate(tc))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
