"""Time the RawNeRF data path's kernels (profiles/rawnerf_data.md).

    python tools/raw_probe.py [--height 3024 --width 4032] [--reps 9] [--no_host]

The demosaic of one uint16 mosaic at n = 1 and n = 4, the post-processing of a 1-MP image, mnr_quantile_f64 on the 3 H W
linear values of the full-resolution frame, and the affine match of a 1-MP pair: HIP events around each call, warm, the
median over `reps` runs.  Next to each: the bytes the call must move, the time those take at the copy rate this project
measured (4.8-5.3 TB/s, profiles/r6_ab.md (c); 5.0 is used), and the same step in NumPy on the host's CPUs (16 threads).
Prints one JSON line.
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

from multinerf_amd import ops, raw_utils  # noqa: E402

COPY_TBPS = 5.0


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


def host_timed(fn, reps=3):
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    ts.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ts))


def host_demosaic(bayer):
  """raw_utils.bilinear_demosaic's closed form with NumPy rolls, float32 (host comparison only)."""
  h, w = bayer.shape
  g = lambda dy, dx: np.roll(bayer, (-dy, -dx), (0, 1))
  out = np.empty((h, w, 3), np.float32)
  ys, xs = np.meshgrid(np.arange(h) % 2, np.arange(w) % 2, indexing='ij')
  cross = .25 * g(0, 1) + .25 * g(0, -1) + .25 * g(1, 0) + .25 * g(-1, 0)
  out[..., 1] = np.where(ys != xs, bayer, cross)
  hor, ver = .5 * (g(0, -1) + g(0, 1)), .5 * (g(-1, 0) + g(1, 0))
  diag = .5 * (.5 * (g(-1, -1) + g(-1, 1)) + .5 * (g(1, -1) + g(1, 1)))
  out[..., 0] = np.select([(ys == 0) & (xs == 0), (ys == 0) & (xs == 1), (ys == 1) & (xs == 0)], [bayer, hor, ver], diag)
  out[..., 2] = np.select([(ys == 1) & (xs == 1), (ys == 1) & (xs == 0), (ys == 0) & (xs == 1)], [bayer, hor, ver], diag)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--height', type=int, default=3024)
  ap.add_argument('--width', type=int, default=4032)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--no_host', action='store_true')
  args = ap.parse_args()
  H, W = args.height, args.width
  rs = np.random.default_rng(0)
  mosaic_h = rs.integers(64, 1024, (1, H, W)).astype(np.uint16)
  mosaic = torch.as_tensor(mosaic_h).cuda()
  black, white = torch.tensor([64.], dtype=torch.float64).cuda(), torch.tensor([1023.], dtype=torch.float64).cuda()
  cam2rgb = np.array([[1.6, -0.4, -0.2], [-0.3, 1.5, -0.2], [0.0, -0.5, 1.5]])
  out = dict(height=H, width=W, reps=args.reps, copy_tbps=COPY_TBPS)
  ideal = lambda nbytes: nbytes / (COPY_TBPS * 1e12) * 1e3

  full = torch.empty((1, H, W, 3), dtype=torch.float32, device='cuda')
  out['demosaic_n1_ms'] = timed(lambda: ops.raw_demosaic(mosaic, black, white, 1.0, 1, out=full), args.reps)
  out['demosaic_n1_bytes'] = H * W * (2 + 12)
  out['demosaic_n1_ms_at_copy_rate'] = ideal(out['demosaic_n1_bytes'])
  quarter = torch.empty((1, H // 4, W // 4, 3), dtype=torch.float32, device='cuda')
  out['demosaic_n4_ms'] = timed(lambda: ops.raw_demosaic(mosaic, black, white, 1.0, 4, out=quarter), args.reps)
  out['demosaic_n4_bytes'] = H * W * 2 + (H // 4) * (W // 4) * 12
  out['demosaic_n4_ms_at_copy_rate'] = ideal(out['demosaic_n4_bytes'])

  P = 1024 * 1024
  img = torch.rand((1024, 1024, 3), device='cuda') * 0.5
  out['postprocess_1mp_f32_u8_ms'] = timed(lambda: ops.raw_postprocess(img, cam2rgb.reshape(-1), 0.4, want=('f32', 'u8')), args.reps)
  out['postprocess_1mp_bytes'] = P * (12 + 12 + 3)
  out['postprocess_1mp_ms_at_copy_rate'] = ideal(out['postprocess_1mp_bytes'])
  img64 = img.double()
  out['postprocess_1mp_f64_ms'] = timed(lambda: ops.raw_postprocess(img64, cam2rgb.reshape(-1), 0.4), args.reps)

  lin = ops.raw_postprocess(full, cam2rgb.reshape(-1), linear_only=True)
  out['quantile_values'] = lin.numel()
  out['quantile_f64_ms'] = timed(lambda: ops.quantile_f64(lin, 97.), args.reps)
  out['quantile_f64_bytes'] = lin.numel() * 8 * 9                   # eight histogram passes and the pass for the next key
  out['quantile_f64_ms_at_copy_rate'] = ideal(out['quantile_f64_bytes'])
  out['quantile_f64_value'] = float(ops.quantile_f64(lin, 97.).cpu()[0])

  est, gt = img64, (img64 * 0.9 + 0.02).contiguous()
  out['affine_match_1mp_ms'] = timed(lambda: raw_utils.match_images_affine(est, gt), args.reps)
  out['affine_sums_1mp_ms'] = timed(lambda: ops.affine_sums(est, gt), args.reps)
  out['affine_apply_1mp_ms'] = timed(lambda: ops.affine_apply(est, [1., 1., 1.], [0., 0., 0.]), args.reps)
  out['affine_match_1mp_bytes'] = P * 24 * 4                        # the sums read two images, the apply reads one and writes one
  out['affine_match_1mp_ms_at_copy_rate'] = ideal(out['affine_match_1mp_bytes'])

  if not args.no_host:
    torch.set_num_threads(16)
    norm = ((mosaic_h[0].astype(np.float32) - 64.) / (1023. - 64.)).astype(np.float32)
    out['host_demosaic_n1_ms'] = host_timed(lambda: host_demosaic(norm), 1)
    lin_h = lin.cpu().numpy()
    out['host_percentile_ms'] = host_timed(lambda: np.percentile(lin_h, 97), 1)
    out['quantile_f64_abs_diff_to_numpy'] = abs(float(np.percentile(lin_h, 97)) - out['quantile_f64_value'])
    img_h = img64.cpu().numpy()
    eps = float(np.finfo(np.float32).eps)

    def host_post():
      z = np.clip(img_h @ cam2rgb.T / 0.4, 0, 1)
      return np.where(z <= 0.0031308, 323 / 25 * z, (211 * np.maximum(eps, z)**(5 / 12) - 11) / 200)

    out['host_postprocess_1mp_ms'] = host_timed(host_post)
    gt_h = gt.cpu().numpy()

    def host_affine():
      x_m, y_m = gt_h.mean((0, 1)), img_h.mean((0, 1))
      a = ((gt_h * img_h).mean((0, 1)) - x_m * y_m) / ((gt_h * gt_h).mean((0, 1)) - x_m * x_m)
      return (img_h - (y_m - a * x_m)) / a

    out['host_affine_match_1mp_ms'] = host_timed(host_affine)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
