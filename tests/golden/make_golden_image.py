#!/usr/bin/env python
"""Record the reference's own image functions (internal/image.py) on seeded images.

    python tests/golden/make_golden_image.py            # writes tests/golden/image_metrics.npz

The reference module is imported FROM WHERE IT LIES (MULTINERF_REFERENCE, nothing is copied) on the NumPy stand-in of
tests/golden/make_golden.py (float64).  Two things the stand-in lacks are supplied here: `jax.jit` (identity) and a stub
`dm_pix` module whose `ssim` is the float64 restatement of tests/image_ref.py (dm_pix is neither installed nor part of
the reference tree; its definition is restated there and cross-checked in tests/test_image_cpu.py).

Per case the file holds the two images (float16, so float32-representable), and from the reference in float64:
`color_correct(img, ref)`; MetricHarness on the plain and on the corrected image, prepared as eval.py:134-146 prepares
them, for every (quantise, crop) combination of the case; for the first case also linear_to_srgb / srgb_to_linear /
downsample.  Cases: a colour-cast, gamma-shifted, noisy image with clipped regions in both images (all three mask terms of
image.py:111 decide pixels on their own); a grey image against a grey reference (the system is rank deficient); an image identical to its
reference; a size that is no multiple of any tile (75 x 93); a crop case.

The generator walks seeds until, in EVERY case, no pre-quantisation value of the corrected image lies within 1e-6 of a
rounding tie (k + 0.5) / 255, and no value the masks test (any iterate of the corrected image, the reference image) lies
within 1e-9 of eps or 1 - eps: no comparison can flip for rounding reasons.  It asserts both.  A window of 2e-6 around
256 ties catches a handful of an image's ~1e4 values under any seed, so within a seed the input pixels behind the
offending values are moved by one float16 step and the case is recomputed, until none is left (a few rounds; a seed
that does not get there in 40 is dropped).  The .npz holds arrays only.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402

OUT = os.path.join(HERE, 'image_metrics.npz')
EPS = 0.5 / 255

# name: kind, height, width, crops (0 = none) the metrics are recorded with
CASES = {
    'cast': dict(kind='cast', H=64, W=80, crops=(0,)),
    'grey': dict(kind='grey', H=40, W=48, crops=(0,)),
    'identical': dict(kind='identical', H=32, W=40, crops=(0,)),
    'odd': dict(kind='cast', H=75, W=93, crops=(0,)),
    'crop': dict(kind='cast', H=48, W=64, crops=(0, 6)),
}


def to_f16(x):
  x = np.clip(x, 0, 1).astype(np.float16)
  x[x == np.float16(0.5)] = np.nextafter(np.float16(0.5), np.float16(1))     # 0.5 * 255 is a rounding tie by itself
  return x


def make_images(rs, c):
  H, W = c['H'], c['W']
  yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing='ij')
  ref = np.zeros((H, W, 3))
  for ch in range(3):
    f = rs.uniform(1.0, 4.0, 4)
    p = rs.uniform(0, 2 * np.pi, 2)
    # amplitude past [0, 1]: the reference image has saturated regions of its own
    ref[..., ch] = 0.5 + 0.42 * np.sin(2 * np.pi * (f[0] * xx + f[1] * yy) + p[0]) + 0.2 * np.sin(2 * np.pi * (f[2] * xx - f[3] * yy) + p[1])
  ref = to_f16(ref).astype(np.float64)
  if c['kind'] == 'identical':
    return to_f16(ref), to_f16(ref)
  if c['kind'] == 'grey':
    # both images grey: every iterate keeps r = g = b exactly, the ten columns span three dimensions, and the minimum-norm
    # solution is well defined (a grey image against a coloured one turns the SECOND iteration's system into a numerically
    # rank-deficient one, whose lstsq solution hangs on rounding noise in the reference itself)
    lum_ref = ref[..., 1]
    lum = np.maximum(lum_ref, 0) ** rs.uniform(0.7, 1.4) * rs.uniform(0.8, 1.2) + rs.uniform(-0.05, 0.05) + 0.02 * rs.standard_normal((H, W))
    return to_f16(np.repeat(lum[..., None], 3, -1)), to_f16(np.repeat(lum_ref[..., None], 3, -1))
  # colour cast (a near-diagonal matrix), gamma, offset, noise; gains past 1 saturate parts of the image itself
  M = np.diag(rs.uniform(0.75, 1.3, 3)) + 0.08 * rs.standard_normal((3, 3))
  img = (np.maximum(ref, 0) ** rs.uniform(0.7, 1.4)) @ M + rs.uniform(-0.06, 0.06, 3) + 0.015 * rs.standard_normal((H, W, 3))
  return to_f16(img), to_f16(ref)


def tie_distance(cc):
  """Distance of every value to the nearest rounding tie (k + 0.5) / 255."""
  frac = cc * 255 - np.floor(cc * 255)
  return np.abs(frac - 0.5) / 255


def try_case(name, c, seed, image, ref_fns):
  rs = np.random.RandomState(seed)
  img16, ref16 = make_images(rs, c)
  for _ in range(40):
    img, gt = img16.astype(np.float64), ref16.astype(np.float64)
    cc = np.asarray(image.color_correct(img, gt), np.float64)
    bad = tie_distance(cc) <= 2e-6                             # (twice the asserted margin)
    if not bad.any():
      break
    px = bad.any(-1)                                           # move the whole pixel: a grey image stays grey
    step = np.where(img16[px] < np.float16(0.5), np.float16(1), np.float16(0))
    img16[px] = np.nextafter(img16[px], step)
    img16 = to_f16(img16)
    if c['kind'] == 'identical':
      ref16 = img16.copy()
  else:
    return None
  # the margins, on the step-by-step restatement's iterates (equal to the reference's to ~1e-13, asserted below)
  trace = []
  own = ref_fns.color_correct(img, gt, trace=trace)
  assert np.abs(own - cc).max() < 1e-9, (name, np.abs(own - cc).max())
  tested = np.concatenate([t[0].ravel() for t in trace] + [gt.ravel()])
  if min(np.abs(tested - EPS).min(), np.abs(tested - (1 - EPS)).min()) <= 1e-9:
    return None
  if tie_distance(cc).min() <= 1e-6:
    return None
  if name == 'cast':
    # each of the three mask terms of image.py:111 removes pixels the other two would keep
    alone = [0, 0, 0]
    for _, m0, cur, refu in trace:
      alone[0] += int((~m0 & cur & refu).sum())
      alone[1] += int((m0 & ~cur & refu).sum())
      alone[2] += int((m0 & cur & ~refu).sum())
    if min(alone) == 0:
      return None
  harness = image.MetricHarness()
  out = {'img': img16, 'ref': ref16, 'cc': cc, 'seed': np.int64(seed), 'crops': np.array(c['crops'], np.int64)}
  for crop in c['crops']:
    for quant in (0, 1):
      for tag, pred in (('metric', img), ('metric_cc', cc)):
        p, g = pred, gt
        if quant:
          p = np.round(p * 255) / 255                                      # eval.py:134-137
        if crop > 0:
          p, g = p[crop:-crop, crop:-crop], g[crop:-crop, crop:-crop]      # :139-143
        m = harness(p, g)
        out[f'{tag}/q{quant}c{crop}'] = np.array([m['psnr'], m['ssim']], np.float64)
  if name == 'cast':
    out['linear_to_srgb'] = np.asarray(image.linear_to_srgb(img, xnp=np), np.float64)
    out['srgb_to_linear'] = np.asarray(image.srgb_to_linear(img, xnp=np), np.float64)
    out['downsample4'] = np.asarray(image.downsample(img, 4), np.float64)
  return out


def main():
  jax = make_golden.install_jax_standin()
  jax.jit = lambda f: f
  from tests import image_ref
  sys.modules['dm_pix'].ssim = image_ref.ssim
  sys.path.insert(0, make_golden.REF)
  from internal import image
  out = {}
  for k, (name, c) in enumerate(CASES.items()):
    for seed in range(1000 * (k + 1), 1000 * (k + 1) + 200):
      g = try_case(name, c, seed, image, image_ref)
      if g is not None:
        break
    assert g is not None, f'{name}: no seed keeps every value clear of the rounding ties and of eps / 1 - eps'
    for key, v in g.items():
      out[f'{name}/{key}'] = v
    print(f"{name}: seed {int(g['seed'])}, plain {np.round(g['metric/q1c0'], 4)}, corrected {np.round(g['metric_cc/q1c0'], 4)}")
  np.savez_compressed(OUT, **out)
  print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes)')


if __name__ == '__main__':
  main()
