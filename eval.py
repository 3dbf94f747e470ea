#!/usr/bin/env python
"""Evaluation script (reference eval.py:40-260, minus TensorBoard / LPIPS / vis): restore the latest checkpoint, render
the test set, and score every image as the reference does (multinerf_amd.image.evaluate_image: colour correction, 8-bit
quantisation, border crop, PSNR + SSIM, disparity and normal metrics, all on the device).

Under <checkpoint_dir>/test_preds it writes metric_<name>_<step>.txt, metric_cc_<name>_<step>.txt and
render_times_<step>.txt, color_NNN.png for every image, and for every Config.eval_render_interval-th image
color_cc_NNN.png, distance_mean / distance_median / acc TIFFs (32-bit float) and normals_NNN.png.  With
Config.eval_quantize_metrics the colour PNGs hold exactly the 8-bit values the metrics were taken on.

  python eval.py --gin_configs configs/blender_256.gin --gin_bindings "Config.data_dir = '...'" \
      --gin_bindings "Config.checkpoint_dir = '...'"
"""

import argparse
import json
import math
import os
import time

import numpy as np
import torch

from multinerf_amd import checkpoints, configs, datasets, image, models, train_utils
from multinerf_amd import dist as mdist


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gin_configs', action='append', default=[])
  ap.add_argument('--gin_bindings', action='append', default=[])
  ap.add_argument('--preset', default=None)
  args = ap.parse_args()
  mdist.init_from_env()
  rank, world = mdist.rank(), mdist.world_size()
  dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
  torch.cuda.set_device(dev)
  config = configs.load_preset(args.preset, args.gin_bindings) if args.preset else \
      configs.load_config(args.gin_configs, args.gin_bindings, save_config=False)
  if config.eval_raw_affine_cc and not config.rawnerf_mode:
    raise SystemExit('eval.py: Config.eval_raw_affine_cc = True needs Config.rawnerf_mode (raw_utils.match_images_affine is '
                     'meant for the raw test scenes); the quadratic image.color_correct is used otherwise')
  dataset = datasets.load_dataset('test', config.data_dir, config, device=dev)
  postprocess_fn = dataset.metadata['postprocess_fn'] if config.rawnerf_mode else None          # eval.py:57-60
  model, state, render_eval_pfn, _, _ = train_utils.setup_model(config, 20200823, dataset=dataset, device=dev)
  if not config.checkpoint_dir or not os.path.isdir(config.checkpoint_dir):
    raise SystemExit(f'eval.py: Config.checkpoint_dir = {config.checkpoint_dir!r} is not a directory')
  if checkpoints.latest_checkpoint(config.checkpoint_dir) is None:
    # (the reference polls until train.py writes one, eval.py:92-104; evaluating random-init weights is never wanted)
    raise SystemExit(f'eval.py: no checkpoint in {config.checkpoint_dir}')
  state = checkpoints.restore_checkpoint(config.checkpoint_dir, model, state)
  step = int(state.step)
  if rank == 0:
    print(f'Evaluating checkpoint at step {step}.')
  out_dir = os.path.join(config.checkpoint_dir, 'test_preds') if config.checkpoint_dir else None
  if out_dir and config.eval_save_output and rank == 0:
    os.makedirs(out_dir, exist_ok=True)
  psnrs, metrics, metrics_cc, render_times = [], [], [], []
  metric_harness = image.MetricHarness()
  save = bool(out_dir and config.eval_save_output)

  def save_u8(x, name):                                        # utils.save_img_u8's range, rounded to nearest
    from PIL import Image
    Image.fromarray((x.clamp(0, 1).cpu().numpy() * 255 + 0.5).astype(np.uint8)).save(os.path.join(out_dir, name))

  def save_f32(x, name):                                       # utils.save_img_f32
    from PIL import Image
    Image.fromarray(np.nan_to_num(x.cpu().numpy()).astype(np.float32)).save(os.path.join(out_dir, name), 'TIFF')

  n = min(dataset.size, config.eval_dataset_limit)
  for idx in range(n):
    batch = next(dataset)
    t0 = time.time()
    rendering = models.render_image(lambda rng, r: render_eval_pfn(state.params, 1.0, None, r), batch.rays, None,
                                    config, verbose=False, world_size=world, rank=rank)
    torch.cuda.synchronize()
    if rank != 0:
      continue
    render_times.append(time.time() - t0)
    pp = postprocess_fn if postprocess_fn is not None else (lambda z: z)
    mse = float(((pp(rendering['rgb']) - pp(batch.rgb))**2).mean())
    psnr = -10. / math.log(10.) * math.log(max(mse, 1e-30))
    psnrs.append(psnr)
    print(f'Eval image {idx + 1}/{n}: {time.time() - t0:.3f}s, psnr {psnr:.3f}', flush=True)
    t1 = time.time()
    metric, metric_cc, images = image.evaluate_image(rendering, batch, config, metric_harness,
                                                     postprocess_fn=postprocess_fn)               # eval.py:118-163
    print(f'Color corrected and scored in {time.time() - t1:0.3f}s')
    for m, v in metric.items():
      print(f'{m:30s} = {v:.4f}')
    for m, v in metric_cc.items():
      print(f'{"cc_" + m:30s} = {v:.4f}')
    metrics.append(metric)
    metrics_cc.append(metric_cc)
    if save:
      from PIL import Image
      # (eval_quantize_metrics: np.round, the very values the metrics saw; it differs from the + 0.5 form only where
      # float32 rounding of x * 255 crosses a tie)
      to_u8 = image.quantize_u8 if config.eval_quantize_metrics else \
          (lambda x: (x.clamp(0, 1).cpu().numpy() * 255 + 0.5).astype(np.uint8))
      Image.fromarray(to_u8(images['color'])).save(os.path.join(out_dir, f'color_{idx:03d}.png'))
      if config.eval_render_interval > 0 and idx % config.eval_render_interval == 0:             # eval.py:171-188
        Image.fromarray(to_u8(images['color_cc'])).save(os.path.join(out_dir, f'color_cc_{idx:03d}.png'))
        for key in ('distance_mean', 'distance_median', 'acc'):
          if key in images:
            save_f32(images[key], f'{key}_{idx:03d}.tiff')
        if 'normals' in images:
          save_u8(images['normals'] / 2. + 0.5, f'normals_{idx:03d}.png')
  if rank == 0:
    print(f'Average test psnr over {len(psnrs)} images: {np.mean(psnrs):.3f}')
    if out_dir:
      with open(os.path.join(config.checkpoint_dir, f'metric_psnr_{step}.txt'), 'w') as f:
        f.write(' '.join(str(p) for p in psnrs))
    if metrics:
      for name in metrics[0]:
        print(f'{"mean_" + name:30s} = {np.mean([m[name] for m in metrics]):.4f}')
      for name in metrics_cc[0]:
        print(f'{"mean_cc_" + name:30s} = {np.mean([m[name] for m in metrics_cc]):.4f}')
    if save and metrics:                                                                           # eval.py:227-236
      with open(os.path.join(out_dir, f'render_times_{step}.txt'), 'w') as f:
        f.write(' '.join(str(r) for r in render_times))
      for name in metrics[0]:
        with open(os.path.join(out_dir, f'metric_{name}_{step}.txt'), 'w') as f:
          f.write(' '.join(str(m[name]) for m in metrics))
      for name in metrics_cc[0]:
        with open(os.path.join(out_dir, f'metric_cc_{name}_{step}.txt'), 'w') as f:
          f.write(' '.join(str(m[name]) for m in metrics_cc))
  mdist.barrier()


if __name__ == '__main__':
  main()
