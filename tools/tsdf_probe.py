"""Time the TSDF fusion kernel (profiles/tsdf_mesh.md).

    python tools/tsdf_probe.py [--reps 9] [--sizes 256,512] [--frames 16]

16 synthetic frames of 1024 x 768 of the sphere |x| = 0.6 (z-depth, acc, colour; cameras on two rings at distance 2.5) are
fused into n^3 volumes over [-1, 1]^3 with a truncation of 3 spacings, with and without colour: median HIP-event time of one
mnr_tsdf_integrate call over `reps` after two untimed calls, next to a device-to-device copy in the same process.

"bytes that must move" per call, from the shapes: every volume read and written once (tsdf and weight 16 n^3, colour 24 n^3
more) plus every image once (depth and acc 8 F H W, colour 12 F H W more).  What the gathers really fetch depends on the
caches and is left out.  Prints one JSON line.
"""

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, FOCAL, RADIUS = 768, 1024, 900., 0.6


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


def look_at(c):
  c = np.asarray(c, np.float64)
  fwd = -c / np.linalg.norm(c)
  right = np.cross(fwd, [0., 0., 1.])
  right /= np.linalg.norm(right)
  return np.stack([right, np.cross(right, fwd), -fwd, c], -1)


def frames(F):
  """(proj [F,3,4], depth [F,H,W], acc [F,H,W], rgb [F,H,W,3]) float32 on the device."""
  from multinerf_amd import mesh
  K = np.array([[FOCAL, 0., W / 2.], [0., FOCAL, H / 2.], [0., 0., 1.]])
  pixtocam = torch.as_tensor(np.linalg.inv(K), device='cuda')
  ys, xs = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float64), torch.arange(W, device='cuda', dtype=torch.float64), indexing='ij')
  cam = torch.stack([xs + .5, ys + .5, torch.ones_like(xs)], -1) @ pixtocam.T * torch.tensor([1., -1., -1.], device='cuda', dtype=torch.float64)
  proj, depth, acc, rgb = [], [], [], []
  for n in range(F):
    zrel = -0.5 if n % 2 == 0 else 0.5
    phi = 2. * math.pi * n / F
    rho = math.sqrt(1. - zrel * zrel)
    c2w = look_at((2.5 * rho * math.cos(phi), 2.5 * rho * math.sin(phi), 2.5 * zrel))
    R, o = torch.as_tensor(c2w[:, :3], device='cuda'), torch.as_tensor(c2w[:, 3], device='cuda')
    d = cam @ R.T
    a, b, c = (d * d).sum(-1), d @ o, float(o @ o) - RADIUS * RADIUS
    disc = b * b - a * c
    t = (-b - torch.sqrt(disc.clamp(min=0.))) / a
    hit = (disc > 0) & (t > 0)
    nrm = (o + d * t[..., None]) / RADIUS
    proj.append(torch.as_tensor(mesh.world_to_pixel(np.linalg.inv(K), c2w)).cuda())
    depth.append(torch.where(hit, t, torch.zeros_like(t)).float())
    acc.append(hit.float())
    rgb.append(torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.ones_like(nrm)).float())
  return tuple(torch.stack(x).contiguous() for x in (proj, depth, acc, rgb))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--sizes', default='256,512')
  ap.add_argument('--frames', type=int, default=16)
  args = ap.parse_args()
  from multinerf_amd import ops
  out = dict(reps=args.reps, frames=args.frames, image=[H, W])
  a = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
  b = torch.empty_like(a)
  copy_ms = timed(lambda: b.copy_(a), args.reps)
  copy_gbps = 2 * a.numel() / copy_ms / 1e6
  out['copy_1GiB'] = dict(ms=copy_ms, gbps=copy_gbps)
  del a, b
  proj, depth, acc, rgb = frames(args.frames)
  F = args.frames
  for n in (int(v) for v in args.sizes.split(',')):
    spacing = float(np.float32(2. / (n - 1)))
    N = n ** 3
    res = {}
    for colors in (True, False):
      tsdf = torch.ones((n, n, n), dtype=torch.float32, device='cuda')
      weight = torch.zeros_like(tsdf)
      color = torch.zeros((n, n, n, 3), dtype=torch.float32, device='cuda') if colors else None
      call = lambda: ops.tsdf_integrate(tsdf, weight, color, (-1., -1., -1.), spacing, 3 * spacing, proj, depth, acc=acc,
                                        rgb=rgb if colors else None)
      call()
      res['never_observed'] = int((weight == 0).sum())
      ms = timed(call, args.reps)
      nbytes = (16 + (24 if colors else 0)) * N + (8 + (12 if colors else 0)) * F * H * W
      res['color' if colors else 'bare'] = dict(ms=ms, updates_per_s=N * F / ms * 1e3, bytes=nbytes, gbps=nbytes / ms / 1e6,
                                                of_copy=nbytes / ms / 1e6 / copy_gbps)
      del tsdf, weight, color
      torch.cuda.empty_cache()
    out[f'volume_{n}'] = dict(points=N, **res)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
