"""Time the TSDF fusion kernel (profiles/tsdf_mesh.md).

    python tools/tsdf_probe.py [--reps 9] [--sizes 256,512] [--frames 16] [--camtype pinhole|perspective|fisheye|pano]

16 synthetic frames of 1024 x 768 of the sphere |x| = 0.6 (z-depth, acc, colour; cameras on two rings at distance 2.5) are
fused into n^3 volumes over [-1, 1]^3 with a truncation of 3 spacings, with and without colour: median HIP-event time of one
mnr_tsdf_integrate call over `reps` after two untimed calls, next to a device-to-device copy in the same process.

"bytes that must move" per call, from the shapes: every volume read and written once (tsdf and weight 16 n^3, colour 24 n^3
more) plus every image once (depth and acc 8 F H W, colour 12 F H W more).  What the gathers really fetch depends on the
caches and is left out.  Prints one JSON line.

--camtype (profiles/tsdf_cameras.md) times the general kernel, mnr_tsdf_integrate_cam, on the same scene from the same positions:
`perspective` the same pinhole cameras as records with a mild lens distortion (k1 = -0.05, k2 = 0.004), `fisheye` 900 pixels a
radian, `pano` 768 x 1024 panoramas; the depth is then the distance along the camera's own rays, rendered in float64 torch.  For these
it also reports `culled`, the share of (brick, frame) pairs a host restatement of the kernel's per-brick test drops at each size
(float64, without the rounding margins' float32 arithmetic: a count, not a verdict).  `pinhole`, the default, is the [3,4] kernel
exactly as before.
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


DISTORTION = dict(k1=-0.05, k2=0.004)


def camera_directions(camtype, pixtocam):
  """Camera-space (OpenGL) ray directions [H,W,3] float64 on the device of the pixel centres, as camera_utils builds them: the
  perspective direction has z = -1 (its parameter is the z-depth), fisheye and pano directions have unit length."""
  ys, xs = torch.meshgrid(torch.arange(H, device='cuda', dtype=torch.float64), torch.arange(W, device='cuda', dtype=torch.float64), indexing='ij')
  if camtype == 'pano':
    theta, phi = xs * (2. * math.pi / W), ys * (math.pi / H)
    return torch.stack([-torch.sin(phi) * torch.sin(theta), torch.cos(phi), torch.sin(phi) * torch.cos(theta)], -1)
  p = torch.stack([xs + .5, ys + .5, torch.ones_like(xs)], -1) @ torch.as_tensor(pixtocam, device='cuda').T
  x, y = p[..., 0], p[..., 1]
  if camtype == 'perspective':
    from multinerf_amd import mesh
    k = [DISTORTION.get(n, 0.) for n in ('k1', 'k2', 'k3', 'k4', 'p1', 'p2')]
    ux, uy = mesh._undistort(x.cpu().numpy().ravel(), y.cpu().numpy().ravel(), k)
    x, y = (torch.as_tensor(a.reshape(H, W), device='cuda') for a in (ux, uy))
  if camtype == 'fisheye':
    theta = torch.sqrt(x * x + y * y).clamp(max=math.pi)
    sot = torch.sin(theta) / theta
    return torch.stack([x * sot, -y * sot, -torch.cos(theta)], -1)
  return torch.stack([x, -y, -torch.ones_like(x)], -1)


def frames(F, camtype='pinhole'):
  """(proj [F,3,4] on the device, or for another camtype than 'pinhole' the records [F,28] on the host; depth [F,H,W], acc [F,H,W],
  rgb [F,H,W,3] float32 on the device)."""
  from multinerf_amd import mesh
  K = np.array([[FOCAL, 0., W / 2.], [0., FOCAL, H / 2.], [0., 0., 1.]])
  cam = camera_directions(camtype, np.linalg.inv(K))
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
    if camtype == 'pinhole':
      proj.append(torch.as_tensor(mesh.world_to_pixel(np.linalg.inv(K), c2w)).cuda())
    else:
      proj.append(mesh.camera_record(np.linalg.inv(K), c2w, H, W, distortion_params=DISTORTION if camtype == 'perspective' else None,
                                     camtype=camtype))
    depth.append(torch.where(hit, t, torch.zeros_like(t)).float())
    acc.append(hit.float())
    rgb.append(torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.ones_like(nrm)).float())
  first = torch.stack(proj).contiguous() if camtype == 'pinhole' else np.stack(proj)
  return (first,) + tuple(torch.stack(x).contiguous() for x in (depth, acc, rgb))


def culled_share(records, n, spacing):
  """The share of (brick, frame) pairs that csrc/tsdf.hip's per-brick test for the general kernel drops on the n^3 grid over
  [-1, 1]^3 (bricks of 4 x 8 x 8 voxels), restated on the host in float64 with the kernel's margins.  A count for the profile:
  the kernel's own decisions are not read back, and what shows them harmless is the tests' restatement, which looks at every
  frame for every voxel."""
  model = int(records[0, 25])
  if model == 2:
    return 0.
  lo = lambda size: -1. + spacing * (np.arange((n + size - 1) // size) * size)
  hi = lambda size: -1. + spacing * np.minimum(np.arange((n + size - 1) // size) * size + size - 1, n - 1)
  cx, cy, cz = ((lo(size), hi(size)) for size in (4, 8, 8))
  X0, Y0, Z0 = np.meshgrid(cx[0], cy[0], cz[0], indexing='ij')
  X1, Y1, Z1 = np.meshgrid(cx[1], cy[1], cz[1], indexing='ij')
  centre = np.stack([0.5 * (X0 + X1), 0.5 * (Y0 + Y1), 0.5 * (Z0 + Z1)], -1)
  rho = 1.01 * 0.5 * np.sqrt((X1 - X0) ** 2 + (Y1 - Y0) ** 2 + (Z1 - Z0) ** 2)
  dropped = 0
  for rec in records.astype(np.float64):
    M = rec[:12].reshape(3, 4)
    c = centre @ M[:, :3].T + M[:, 3]
    # the rows' magnitudes at |x|, |y|, |z| = 1, the probe's box: the kernel takes each brick's own largest coordinates, so its
    # margins are these or smaller, and this count is a lower bound by that little
    mags = np.abs(M[:, :3]).sum(1) + np.abs(M[:, 3])
    mag = mags.max()
    r = rho + 1e-5 * mag
    D = np.linalg.norm(c, axis=-1)
    A = np.arctan2(np.hypot(c[..., 0], c[..., 1]), c[..., 2])
    alpha = math.atan(math.sqrt(rec[24])) if model == 0 else math.sqrt(rec[24])
    with np.errstate(invalid='ignore'):
      miss = (D > r) & (A - np.arcsin(np.minimum(r / D, 1.)) > alpha + 1e-3)
    if model == 0:
      behind = np.ones(miss.shape, bool)
      for X in (X0, X1):
        for Y in (Y0, Y1):
          for Z in (Z0, Z1):
            behind &= (M[2, 0] * X + M[2, 1] * Y + M[2, 2] * Z + M[2, 3]) < -1e-6 * mags[2]
      miss |= behind
    dropped += int(miss.sum())
  return dropped / (len(records) * centre[..., 0].size)


def parse_args(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--sizes', default='256,512')
  ap.add_argument('--frames', type=int, default=16)
  ap.add_argument('--camtype', choices=('pinhole', 'perspective', 'fisheye', 'pano'), default='pinhole',
                  help='pinhole: the [3,4] kernel; the others: the general kernel on camera records of that model')
  return ap.parse_args(argv)


def main():
  args = parse_args()
  from multinerf_amd import ops
  out = dict(reps=args.reps, frames=args.frames, image=[H, W], camtype=args.camtype)
  a = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
  b = torch.empty_like(a)
  copy_ms = timed(lambda: b.copy_(a), args.reps)
  copy_gbps = 2 * a.numel() / copy_ms / 1e6
  out['copy_1GiB'] = dict(ms=copy_ms, gbps=copy_gbps)
  del a, b
  proj, depth, acc, rgb = frames(args.frames, args.camtype)
  integrate = ops.tsdf_integrate if args.camtype == 'pinhole' else ops.tsdf_integrate_cam
  F = args.frames
  for n in (int(v) for v in args.sizes.split(',')):
    spacing = float(np.float32(2. / (n - 1)))
    N = n ** 3
    res = {}
    for colors in (True, False):
      tsdf = torch.ones((n, n, n), dtype=torch.float32, device='cuda')
      weight = torch.zeros_like(tsdf)
      color = torch.zeros((n, n, n, 3), dtype=torch.float32, device='cuda') if colors else None
      call = lambda: integrate(tsdf, weight, color, (-1., -1., -1.), spacing, 3 * spacing, proj, depth, acc=acc, rgb=rgb if colors else None)
      call()
      res['never_observed'] = int((weight == 0).sum())
      ms = timed(call, args.reps)
      nbytes = (16 + (24 if colors else 0)) * N + (8 + (12 if colors else 0)) * F * H * W
      res['color' if colors else 'bare'] = dict(ms=ms, updates_per_s=N * F / ms * 1e3, bytes=nbytes, gbps=nbytes / ms / 1e6,
                                                of_copy=nbytes / ms / 1e6 / copy_gbps)
      del tsdf, weight, color
      torch.cuda.empty_cache()
    if args.camtype != 'pinhole':
      res['culled'] = culled_share(proj, n, spacing)
    out[f'volume_{n}'] = dict(points=N, **res)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
