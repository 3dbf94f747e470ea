#!/usr/bin/env python
"""Render script (reference render.py:41-194, minus the mp4 encoder): restore the latest checkpoint and render every
camera of the test split, or with Config.render_path the camera path (spiral / ellipse / spline /
Config.render_path_file, datasets.py).

Under <Config.render_dir or checkpoint_dir/render>/<path_renders|test_preds>_step_<step> it writes per frame
color_NNN.png, normals_NNN.png (when the model has normals) and distance_mean / distance_median / acc TIFFs (32-bit
float); with --vis also every image of multinerf_amd.vis.visualize_suite as vis_<key>_NNN.png.  Frames are strided over
Config.render_num_jobs processes (this one renders those with idx % render_num_jobs == render_job_id), and a frame is
skipped when its own and this job's next colour image both exist.

Video frames.  There is no video encoder here, so what the reference would feed to one is written as PNGs to
<base_dir>/<scene>_<exp>_<out_name>_<k>/NNN.png for k in color, normals, acc, distance_mean, distance_median: colour and
normals as saved, acc as grey, the distances through Config.render_dist_curve_fn, normalised between the
render_dist_percentile-th and (100 - render_dist_percentile)-th percentile of frame 0's distance_mean, and the turbo
colour map.  The percentiles (mnr_quantile) and the colour map (mnr_vis_cmap) run on the device while the frame is still
there; a frame whose limits are not known yet (another job renders frame 0) is colourised from its TIFF once all files
of all jobs exist.  Encoding them: e.g. `ffmpeg -framerate 60 -i %03d.png -crf 18 out.mp4`.

  python render.py --gin_configs configs/360.gin --gin_bindings "Config.data_dir = '...'" \
      --gin_bindings "Config.checkpoint_dir = '...'" --gin_bindings "Config.render_path = True"
"""

import argparse
import concurrent.futures
import glob
import os
import time

import numpy as np
import torch

from multinerf_amd import checkpoints, configs, datasets, models, ops, train_utils, vis
from multinerf_amd import dist as mdist

VIDEO_KEYS = ('color', 'normals', 'acc', 'distance_mean', 'distance_median')
_CURVES = {None: None, 'identity': None, 'log': 'ln'}          # Config.render_dist_curve_fn -> mnr_vis_cmap's curve


def _save_png(arr, path):
  from PIL import Image
  Image.fromarray(arr).save(path, 'PNG')


def _save_tiff(arr, path):
  from PIL import Image
  Image.fromarray(arr).save(path, 'TIFF')


def to_u8(x):
  """utils.save_img_u8's quantisation of a device image, (clip(nan_to_num(x), 0, 1) * 255) truncated, as a host array."""
  return (torch.clamp(torch.nan_to_num(x.to(torch.float32)), 0., 1.) * 255.).to(torch.uint8).cpu().numpy()


def to_f32(x):
  """utils.save_img_f32's array of a device image."""
  return torch.nan_to_num(x.to(torch.float32)).cpu().numpy()


class VideoFrames:
  """The frames create_videos (render.py:41-95) would hand to the encoder, one folder per tag."""

  def __init__(self, config, base_dir, out_dir, out_name, num_frames, save_fn, device, cmaps):
    names = [n for n in config.checkpoint_dir.split('/') if n]
    exp_name, scene_name = (['', ''] + names)[-2:]                # the last two parts of the checkpoint path
    self.prefix = os.path.join(base_dir, f'{scene_name}_{exp_name}_{out_name}')
    self.config, self.out_dir, self.num_frames, self.save_fn, self.device = config, out_dir, num_frames, save_fn, device
    zpad = max(3, len(str(num_frames - 1)))
    self.idx_to_str = lambda idx: str(idx).zfill(zpad)
    if config.render_dist_curve_fn not in _CURVES:
      raise SystemExit(f'render.py: Config.render_dist_curve_fn = {config.render_dist_curve_fn!r}: one of {sorted(map(str, _CURVES))}')
    self.curve = _CURVES[config.render_dist_curve_fn]
    self.turbo = vis.colormap_lut(cmaps.get('turbo', 'turbo'), device)
    self.lohi = None

  def path(self, k, idx):
    return os.path.join(f'{self.prefix}_{k}', f'{self.idx_to_str(idx)}.png')

  def limits(self, distance_mean0=None):
    """(lo, hi) as a device pair: np.percentile of frame 0's distance_mean at p and 100 - p (render.py:54-59); the
    curve is applied to them inside the colour-map kernel.  None while frame 0 is neither given nor on disk."""
    if self.lohi is None:
      if distance_mean0 is None:
        file0 = os.path.join(self.out_dir, f'distance_mean_{self.idx_to_str(0)}.tiff')
        if not os.path.exists(file0):
          return None
        from PIL import Image
        distance_mean0 = torch.as_tensor(np.array(Image.open(file0), dtype=np.float32)).to(self.device)
      d = torch.nan_to_num(distance_mean0.to(torch.float32)).reshape(-1).contiguous()
      p = self.config.render_dist_percentile
      self.lohi = torch.cat([ops.quantile(d, p / 100.), ops.quantile(d, (100. - p) / 100.)])
    return self.lohi

  def colourise(self, distance):
    """One distance image -> the [H,W,3] uint8 device frame (render.py:88-93)."""
    d = torch.nan_to_num(distance.to(torch.float32)).contiguous()
    out = torch.empty(tuple(d.shape[:2]) + (3,), dtype=torch.uint8, device=d.device)
    return ops.vis_cmap(d, self.limits(), curve=self.curve, lut=self.turbo, out_u8=out, want_f32=False)

  def write(self, idx, images):
    """images: {tag: host uint8 array (color, normals) or device float image (acc, distance_*)}; returns the tags left out
    because the distance limits are not known yet."""
    deferred = []
    for k, img in images.items():
      os.makedirs(f'{self.prefix}_{k}', exist_ok=True)
      if k.startswith('distance'):
        if self.limits(img if (idx == 0 and k == 'distance_mean') else None) is None:
          deferred.append(k)
          continue
        img = self.colourise(img).cpu().numpy()
      elif k == 'acc':
        img = to_u8(img)
      self.save_fn(_save_png, img, self.path(k, idx))
    return deferred

  def fill_missing(self):
    """Once every job's files exist: the frames no job could write (or that were lost), from the saved images."""
    from PIL import Image
    for k in VIDEO_KEYS:
      ext = 'png' if k in ('color', 'normals') else 'tiff'
      if not os.path.exists(os.path.join(self.out_dir, f'{k}_{self.idx_to_str(0)}.{ext}')):
        print(f'Images missing for tag {k}')
        continue
      for idx in range(self.num_frames):
        src = os.path.join(self.out_dir, f'{k}_{self.idx_to_str(idx)}.{ext}')
        if os.path.exists(self.path(k, idx)):
          continue
        if not os.path.exists(src):
          raise ValueError(f'Image file {src} does not exist.')
        img = np.array(Image.open(src))
        if ext == 'tiff':
          img = torch.as_tensor(img.astype(np.float32)).to(self.device)
        self.write(idx, {k: img})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gin_configs', action='append', default=[])
  ap.add_argument('--gin_bindings', action='append', default=[])
  ap.add_argument('--preset', default=None)
  ap.add_argument('--vis', action='store_true', help='also write every image of vis.visualize_suite as vis_<key>_NNN.png')
  ap.add_argument('--colormaps', default=None, help='an .npz of [n,3] tables named like the colormaps they replace (turbo, gray)')
  args = ap.parse_args()
  mdist.init_from_env()
  rank, world = mdist.rank(), mdist.world_size()
  dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
  torch.cuda.set_device(dev)
  config = configs.load_preset(args.preset, args.gin_bindings) if args.preset else \
      configs.load_config(args.gin_configs, args.gin_bindings, save_config=False)
  cmaps = {}
  if args.colormaps:
    with np.load(args.colormaps) as z:
      cmaps = {k: torch.as_tensor(z[k].astype(np.float32)).to(dev) for k in z.files}
  dataset = datasets.load_dataset('test', config.data_dir, config, device=dev)
  postprocess_fn = dataset.metadata['postprocess_fn'] if config.rawnerf_mode else None          # render.py:107-110
  model, state, render_eval_pfn, _, _ = train_utils.setup_model(config, 20200823, dataset=dataset, device=dev)
  if not config.checkpoint_dir or checkpoints.latest_checkpoint(config.checkpoint_dir) is None:
    raise SystemExit(f'render.py: no checkpoint in Config.checkpoint_dir = {config.checkpoint_dir!r}')
  state = checkpoints.restore_checkpoint(config.checkpoint_dir, model, state)
  step = int(state.step)
  if rank == 0:
    print(f'Rendering checkpoint at step {step}.')

  out_name = 'path_renders' if config.render_path else 'test_preds'
  out_name = f'{out_name}_step_{step}'
  base_dir = config.render_dir
  if base_dir is None:
    base_dir = os.path.join(config.checkpoint_dir, 'render')
  out_dir = os.path.join(base_dir, out_name)
  if rank == 0:
    os.makedirs(out_dir, exist_ok=True)
  path_fn = lambda x: os.path.join(out_dir, x)

  # Ensure sufficient zero-padding of image indices in output filenames.
  zpad = max(3, len(str(dataset.size - 1)))
  idx_to_str = lambda idx: str(idx).zfill(zpad)

  async_executor, async_futures = None, []
  if config.render_save_async:
    # (the device -> host copy is done by the caller, on the main thread; the pool encodes and writes)
    async_executor = concurrent.futures.ThreadPoolExecutor(max_workers=4)

    def save_fn(fn, *a, **k):
      async_futures.append(async_executor.submit(fn, *a, **k))
  else:
    def save_fn(fn, *a, **k):
      fn(*a, **k)

  video = VideoFrames(config, base_dir, out_dir, out_name, dataset.size, save_fn, dev, cmaps) if rank == 0 else None

  for idx in range(dataset.size):
    if idx % config.render_num_jobs != config.render_job_id:
      continue
    # If current image and next image both already exist, skip ahead.
    idx_str = idx_to_str(idx)
    curr_file = path_fn(f'color_{idx_str}.png')
    next_file = path_fn(f'color_{idx_to_str(idx + config.render_num_jobs)}.png')
    if os.path.exists(curr_file) and os.path.exists(next_file):
      if rank == 0:
        print(f'Image {idx}/{dataset.size} already exists, skipping')
      continue
    if rank == 0:
      print(f'Evaluating image {idx+1}/{dataset.size}')
    eval_start_time = time.time()
    rays = dataset.generate_ray_batch(idx).rays
    rendering = models.render_image(lambda rng, r: render_eval_pfn(state.params, 1.0, None, r), rays, None, config,
                                    verbose=False, world_size=world, rank=rank)
    torch.cuda.synchronize()
    if rank != 0:  # Only record via rank 0.
      continue
    print(f'Rendered in {(time.time() - eval_start_time):0.3f}s', flush=True)

    if postprocess_fn is not None:                                 # render.py:163: raw space -> sRGB, before anything is saved
      rendering['rgb'], rgb_u8 = postprocess_fn(rendering['rgb'].float(), want=('f32', 'u8'))
      frames = {'color': rgb_u8.cpu().numpy()}                     # (the kernel's 8-bit output: utils.save_img_u8's truncation)
    else:
      frames = {'color': to_u8(rendering['rgb'])}
    save_fn(_save_png, frames['color'], path_fn(f'color_{idx_str}.png'))
    if rendering.get('normals') is not None:
      frames['normals'] = to_u8(rendering['normals'] / 2. + 0.5)
      save_fn(_save_png, frames['normals'], path_fn(f'normals_{idx_str}.png'))
    for key in ('distance_mean', 'distance_median', 'acc'):
      save_fn(_save_tiff, to_f32(rendering[key]), path_fn(f'{key}_{idx_str}.tiff'))
      frames[key] = rendering[key]
    video.write(idx, frames)
    if args.vis:
      for key, img in vis.visualize_suite(rendering, rays, cmaps=cmaps).items():
        save_fn(_save_png, to_u8(img), path_fn(f'vis_{key}_{idx_str}.png'))

  if async_executor is not None:
    # Wait until all worker threads finish, then raise what they raised.
    async_executor.shutdown(wait=True)
    for future in async_futures:
      future.result()
    async_futures.clear()
    async_executor = None

  num_files = len(glob.glob(path_fn('acc_*.tiff')))
  if rank == 0 and num_files == dataset.size:
    print(f'All files found, creating videos (job {config.render_job_id}).')
    video.save_fn = lambda fn, *a, **k: fn(*a, **k)
    video.fill_missing()
  mdist.barrier()


if __name__ == '__main__':
  main()
