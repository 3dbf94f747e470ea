#!/usr/bin/env python
"""RobustNeRF end to end: equal-step PSNR on CLEAN held-out views when part of the training images carry distractors.

    python tools/robustnerf_psnr.py [--steps 2000] [--batch 4096] [--frac 0.4] [--out FILE.jsonl]

The procedural scene (multinerf_amd/datasets.py Procedural: a shaded sphere on white, 40 training views of 96 x 96) with
one or two bright squares painted into a fraction of the TRAINING images, each at its own place (a transient object that
is in no other view).  The `blender_256` network is trained twice from the same seeds on the same 16 x 16 patches: with
`data_loss_type = 'robustnerf'` (the 360_robustnerf preset's settings: inlier quantile 0.8, 8 x 8 inner patch, 3 x 3
window) and with `'mse'`.  Printed: the test PSNR of both at equal steps, and for the robust run the inlier fraction
(`mask`) and the threshold over time.  A measurement (profiles/robustnerf.md), not a test: nothing is asserted.
"""

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multinerf_amd import configs, datasets, models, train_utils  # noqa: E402


def paint_distractors(images, frac, seed=11):
  """In place: squares of a saturated colour in the first `frac` of a random order of the images."""
  rs = np.random.default_rng(seed)
  n, H, W, _ = images.shape
  hit = rs.permutation(n)[:int(round(frac * n))]
  covered = 0
  for i in hit:
    for _ in range(int(rs.integers(1, 3))):
      s = int(rs.integers(H // 5, H // 3))
      y, x = int(rs.integers(0, H - s)), int(rs.integers(0, W - s))
      images[i, y:y + s, x:x + s] = torch.as_tensor(rs.choice([0.0, 1.0], 3) * [1.0, 0.9, 0.8], dtype=images.dtype, device=images.device)
      covered += s * s
  return sorted(int(i) for i in hit), covered / (n * H * W)


def run(loss_type, args, dev):
  bind = ["Config.dataset_loader = 'procedural'", "Config.batching = 'all_images'", f'Config.batch_size = {args.batch}',
          'Config.patch_size = 16', f'Config.max_steps = {args.steps}', 'Config.lr_delay_steps = 100',
          f"Config.data_loss_type = '{loss_type}'", 'Config.robustnerf_inlier_quantile = 0.8', 'Config.enable_robustnerf_loss = True']
  config = configs.load_preset('blender_256', bind)
  dataset = datasets.load_dataset('train', None, config, device=dev)
  test = datasets.load_dataset('test', None, config, device=dev)
  hit, covered = paint_distractors(dataset.images, args.frac)
  model, state, render_eval_pfn, train_pstep, _ = train_utils.setup_model(config, 20200823, dataset=dataset, device=dev)
  gen = torch.Generator(device=dev).manual_seed(20200823)
  thr = 1.0
  rows, kept = [], []

  def test_psnr(train_frac):
    out = []
    for _ in range(test.size):
      case = next(test)
      r = models.render_image(lambda rng, rays: render_eval_pfn(state.params, train_frac, None, rays), case.rays, None, config, verbose=False)
      out.append(-10.0 / math.log(10.0) * math.log(max(float(((r['rgb'] - case.rgb) ** 2).mean()), 1e-30)))
    return float(np.mean(out))

  for step in range(1, args.steps + 1):
    train_frac = float(np.clip((step - 1) / (config.max_steps - 1), 0, 1))
    state, stats, gen = train_pstep(gen, state, next(dataset), dataset.cameras, train_frac, thr)
    if loss_type == 'robustnerf':
      thr = stats.loss_threshold_device()
      kept.append(stats)
    if step % args.log_every == 0 or step == args.steps:
      row = dict(loss_type=loss_type, step=step, train_psnr=stats.materialize()['psnr'])
      if kept:
        ms = [k.materialize() for k in kept]
        row.update(inlier_fraction=float(np.mean([m['mask'] for m in ms])), loss_threshold=float(np.mean([m['loss_threshold'] for m in ms])),
                   is_inlier_loss=float(np.mean([m['is_inlier_loss'] for m in ms])))
        kept = []
      if step % args.eval_every == 0 or step == args.steps:
        row['test_psnr_clean'] = test_psnr(train_frac)
      rows.append(row)
      print(json.dumps(row), flush=True)
  return dict(loss_type=loss_type, images_with_distractors=hit, pixels_covered=covered, rows=rows)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=2000)
  ap.add_argument('--batch', type=int, default=4096)
  ap.add_argument('--frac', type=float, default=0.4)
  ap.add_argument('--log_every', type=int, default=100)
  ap.add_argument('--eval_every', type=int, default=500)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dev = torch.device('cuda', 0)
  res = [run(t, args, dev) for t in ('robustnerf', 'mse')]
  final = {r['loss_type']: r['rows'][-1]['test_psnr_clean'] for r in res}
  print(json.dumps(dict(final_test_psnr_clean=final, steps=args.steps, batch=args.batch, frac=args.frac,
                        pixels_covered=res[0]['pixels_covered'])), flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      for r in res:
        f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
  main()
