"""Time the image ingest kernel and a Blender scene load (profiles/datasets_ingest.md).

    python tools/ingest_probe.py [--reps 9]                         # mnr_image_ingest against a device-to-device copy
    python tools/ingest_probe.py --load_scene DIR [--package_root P]   # wall time of loading a 100-image 800 x 800 Blender scene

Kernel part: the achieved GB/s (bytes read plus bytes written over the median HIP-event time, warm) of mnr_image_ingest at
(250,1080,1920,3) uint8, n = 1, plain, and (100,800,800,4) uint8, n = 2, white_bg with alpha, each next to a device-to-device
copy that moves the same total bytes (half of them read, half written), timed in the same process.

Load part: writes the synthetic scene into DIR when it is not there (random RGBA PNGs), then times
datasets.load_dataset('train', DIR, blender_256, device='cuda') three times.  --package_root imports multinerf_amd from
another checkout (the parent commit's tree, for the "before" figure).  Prints one JSON line.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def kernel_part(reps):
  from multinerf_amd import ops
  out = dict(reps=reps)
  for tag, shape, n, mode in (('plain_250x1080x1920x3_n1', (250, 1080, 1920, 3), 1, 'plain'),
                              ('white_bg_100x800x800x4_n2', (100, 800, 800, 4), 2, 'white_bg')):
    N, H, W, C = shape
    src = torch.randint(0, 256, shape, dtype=torch.uint8, device='cuda')
    dst = torch.empty((N, H // n, W // n, 3), dtype=torch.float32, device='cuda')
    alpha = torch.empty((N, H // n, W // n), dtype=torch.float32, device='cuda') if mode == 'white_bg' else None
    nbytes = src.numel() + dst.numel() * 4 + (alpha.numel() * 4 if alpha is not None else 0)
    ms = timed(lambda: ops.image_ingest(src, n, mode, out=dst, alpha=alpha), reps)
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
    b = torch.empty_like(a)
    copy_ms = timed(lambda: b.copy_(a), reps)
    out[tag] = dict(bytes=nbytes, ms=ms, gbps=nbytes / ms / 1e6, copy_ms=copy_ms, copy_gbps=2 * a.numel() / copy_ms / 1e6,
                    ratio=copy_ms / ms)
    del src, dst, alpha, a, b
    torch.cuda.empty_cache()
  return out


def load_part(scene, reps=3):
  from PIL import Image
  from multinerf_amd import configs, datasets
  if not os.path.exists(os.path.join(scene, 'transforms_train.json')):
    os.makedirs(os.path.join(scene, 'train'), exist_ok=True)
    rs = np.random.default_rng(0)
    frames = []
    for i in range(100):
      Image.fromarray(rs.integers(0, 256, (800, 800, 4), dtype=np.uint8), 'RGBA').save(os.path.join(scene, 'train', f'r_{i}.png'), compress_level=1)
      m = np.eye(4)
      m[:3, 3] = [0.01 * i, 0.2, 4.0]
      frames.append({'file_path': f'./train/r_{i}', 'transform_matrix': m.tolist()})
    with open(os.path.join(scene, 'transforms_train.json'), 'w') as f:
      json.dump({'camera_angle_x': 0.7, 'frames': frames}, f)
  cfg = configs.load_preset('blender_256', ['Config.factor = 0'])
  torch.zeros(1).cuda()
  ts = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = datasets.load_dataset('train', scene, cfg, device='cuda')
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
    checksum = float(ds.images.double().sum())
    del ds
  return dict(package=os.path.dirname(os.path.abspath(datasets.__file__)), load_s=ts, load_s_median=float(np.median(ts)), checksum=checksum)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--load_scene', default=None)
  ap.add_argument('--package_root', default=ROOT)
  args = ap.parse_args()
  sys.path.insert(0, os.path.abspath(args.package_root))
  print(json.dumps(load_part(args.load_scene) if args.load_scene else kernel_part(args.reps)))


if __name__ == '__main__':
  main()
