"""Time the evaluation metrics of one image against its render (profiles/eval_metrics.md).

    python tools/eval_metrics_probe.py [--height 960 --width 1024] [--reps 5] [--no_render] [--no_host]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/eval_metrics_probe.py --no_render --no_host --reps 3

A synthetic colour-cast pair of the given size is scored on the device: mnr_ssim, the statistics pass, one full
image.color_correct (5 iterations: Gram + apply launches and the host's 10 x 10 solves), and image.evaluate_image as
eval.py calls it.  Next to it: the render of an image of the same size by the 360 preset's model at random weights
(models.render_image, the path eval.py takes; the time does not depend on the weights), and the float64 NumPy
restatement of color_correct on the host's CPUs.  Prints one JSON line.
"""

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multinerf_amd import configs, image, models, ops, synthetic, train_utils  # noqa: E402


def make_pair(H, W, seed=0):
  rs = np.random.RandomState(seed)
  yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
  ref = np.stack([0.5 + 0.42 * np.sin(2 * np.pi * (f[0] * xx + f[1] * yy) + f[2]) + 0.2 * np.sin(2 * np.pi * (f[3] * xx - f[0] * yy))
                  for f in rs.uniform(1.0, 6.0, (3, 4))], -1).clip(0, 1)
  M = np.diag(rs.uniform(0.75, 1.3, 3)) + 0.08 * rs.standard_normal((3, 3))
  img = ((ref ** 1.2) @ M + rs.uniform(-0.06, 0.06, 3) + 0.015 * rs.standard_normal((H, W, 3))).clip(0, 1)
  return img.astype(np.float32), ref.astype(np.float32)


def timed(fn, reps):
  """Median wall time in ms of fn() with a device synchronisation on both sides (one untimed call first)."""
  fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ts))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--height', type=int, default=960)
  ap.add_argument('--width', type=int, default=1024)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--no_render', action='store_true')
  ap.add_argument('--no_host', action='store_true')
  args = ap.parse_args()
  H, W = args.height, args.width
  img, ref = make_pair(H, W)
  a, b = torch.as_tensor(img).cuda(), torch.as_tensor(ref).cuda()
  a64, b64 = a.double(), b.double()
  q32 = torch.empty_like(a)
  out = dict(height=H, width=W, reps=args.reps)
  out['ssim_ms'] = timed(lambda: ops.ssim(a, b), args.reps)
  out['sqdiff_ms'] = timed(lambda: ops.image_sqdiff(a64, b64, quantize=True, q_out=q32), args.reps)
  out['color_correct_ms'] = timed(lambda: image.color_correct(a64, b64), args.reps)
  mask0 = torch.empty((H * W, 3), dtype=torch.uint8, device='cuda')
  flat_a, flat_b = a64.reshape(-1, 3), b64.reshape(-1, 3)
  out['cc_gram_ms'] = timed(lambda: ops.cc_gram(flat_a, flat_b, mask0, 0.5 / 255, write_mask0=True), args.reps)
  warp = np.zeros((10, 3))
  warp[6:9] = np.eye(3)
  out['cc_apply_ms'] = timed(lambda: ops.cc_apply(flat_a, warp), args.reps)
  config = configs.Config()
  batch = types.SimpleNamespace(rgb=b)
  harness = image.MetricHarness()
  res = {}

  def evaluate():
    res['m'] = image.evaluate_image({'rgb': a}, batch, config, harness)

  out['evaluate_image_ms'] = timed(evaluate, args.reps)
  out['metric'], out['metric_cc'] = res['m'][0], res['m'][1]
  if not args.no_render:
    cfg = configs.load_preset('360', [])
    model, state, render_eval_pfn, _, _ = train_utils.setup_model(cfg, 20200823, device='cuda')
    rays = synthetic.synthetic_rays(H * W, near=cfg.near, far=cfg.far, device='cuda').rays.map(lambda r: r.reshape(H, W, -1))

    def render():
      models.render_image(lambda rng, r: render_eval_pfn(state.params, 1.0, None, r), rays, None, cfg, verbose=False)

    out['render_ms'] = timed(render, max(1, args.reps // 2))
    out['render_rays_per_sec'] = H * W / (out['render_ms'] * 1e-3)
  if not args.no_host:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import image_ref
    torch.set_num_threads(16)
    t0 = time.perf_counter()
    cc = image_ref.color_correct(img.astype(np.float64), ref.astype(np.float64))
    out['host_color_correct_f64_ms'] = (time.perf_counter() - t0) * 1e3
    dev = image.color_correct(a64, b64).cpu().numpy()
    out['cc_max_abs_diff_to_host'] = float(np.abs(dev - cc).max())
    out['cc_differing_u8'] = int((np.round(dev * 255) != np.round(cc * 255)).sum())
  print(json.dumps(out))


if __name__ == '__main__':
  main()
