#!/usr/bin/env python
"""Record the reference's own RobustNeRF mask (internal/robustnerf.py) on seeded patch batches.

    python tests/golden/make_golden_robustnerf.py            # writes tests/golden/robustnerf.npz and
                                                             # tests/golden/reference_gin_bindings_robustnerf.json

The reference module is imported FROM WHERE IT LIES (MULTINERF_REFERENCE, nothing is copied) on the NumPy stand-in of
tests/golden/make_golden.py (float64).  Two things the stand-in lacks are supplied here: `lax.conv` with 'SAME' padding
(direct sums over the window, NCHW x OIHW with one channel, as robustnerf.py:45-47 calls it), and `jnp.mean` over a LIST of
axes (robustnerf.py:68-70; NumPy wants a tuple).  `jnp.quantile` is NumPy's.

Per case the file holds the inputs (float32-representable: rendered rgb, ground truth, lossmult, the threshold), the
settings, and the reference's outputs in float64: mask, the four means, the next threshold (the quantile), plus
train_utils.py:86-88's mse and lossmult * mask.  Images are a smooth background of small error with a few blobs of large
error, salt noise and clean specks inside the blobs, so that each of the three criteria decides some pixels on its own.

The generator walks seeds until, for EVERY pixel of the case, the per-pixel error is further than a relative 1e-5 from
the threshold (fp32 evaluates a mean of three squared differences to a few 1e-7: no comparison can flip), and no box or
patch vote sits on its tie; it asserts both, and that every criterion fires.  The .npz holds arrays only.

The .json records what the reference's configs/360_robustnerf.gin binds, in the format of reference_gin_bindings.json
(tests/golden/make_golden_gin.py, which stays as it is: its output file is pinned by existing tests).
"""

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402

OUT = os.path.join(HERE, 'robustnerf.npz')
OUT_GIN = os.path.join(HERE, 'reference_gin_bindings_robustnerf.json')

# name: patch, inner, filter, patches, padded B (0: none), lm_c, smoothed q, patch q, inlier q (next threshold), enable,
#       threshold ('mid': a quantile of the case's own errors, else the value)
CASES = {
    'preset':   dict(P=16, inner=8, f=3, patches=64, B=0, lm_c=1, qs=0.5, qp=0.5, qi=0.8, enable=True, thr='mid'),
    'odd':      dict(P=8, inner=3, f=3, patches=32, B=0, lm_c=3, qs=0.5, qp=0.5, qi=0.5, enable=True, thr='mid'),
    'f1':       dict(P=4, inner=4, f=1, patches=16, B=0, lm_c=1, qs=0.5, qp=0.5, qi=0.5, enable=True, thr='mid'),
    'f5':       dict(P=16, inner=7, f=5, patches=16, B=0, lm_c=3, qs=0.5, qp=0.5, qi=0.8, enable=True, thr='mid'),
    'disabled': dict(P=16, inner=8, f=3, patches=8, B=0, lm_c=1, qs=0.5, qp=0.5, qi=0.8, enable=False, thr='mid'),
    'q08':      dict(P=16, inner=8, f=3, patches=16, B=0, lm_c=3, qs=0.8, qp=0.8, qi=0.8, enable=True, thr='mid'),
    'thr0':     dict(P=16, inner=8, f=3, patches=8, B=0, lm_c=1, qs=0.5, qp=0.5, qi=0.8, enable=True, thr=0.0),
    'thrbig':   dict(P=16, inner=8, f=3, patches=8, B=0, lm_c=3, qs=0.5, qp=0.5, qi=0.5, enable=True, thr=1e30),
    'padded':   dict(P=8, inner=4, f=3, patches=5, B=384, lm_c=1, qs=0.5, qp=0.5, qi=0.8, enable=True, thr='mid'),
}


def install_missing(jax):
  jnp = jax.numpy

  def conv(lhs, rhs, window_strides, padding):
    assert padding == 'SAME' and tuple(window_strides) == (1, 1) and lhs.shape[1] == 1 and rhs.shape[:2] == (1, 1)
    fh, fw = rhs.shape[2:]
    H, W = lhs.shape[2:]
    # 'SAME' at stride 1: total padding f - 1, the smaller half in front (equal halves for odd f)
    ph, pw = (fh - 1) // 2, (fw - 1) // 2
    x = np.zeros((lhs.shape[0], H + fh - 1, W + fw - 1), np.float64)
    x[:, ph:ph + H, pw:pw + W] = lhs[:, 0]
    out = np.zeros((lhs.shape[0], H, W), np.float64)
    for i in range(fh):
      for j in range(fw):
        out += rhs[0, 0, i, j] * x[:, i:i + H, j:j + W]
    return out[:, None]

  sys.modules['jax.lax'].conv = conv
  np_mean = np.mean
  jnp.mean = lambda a, axis=None, **kw: np_mean(a, axis=tuple(axis) if isinstance(axis, list) else axis, **kw)
  jnp.ones_like = lambda a, dtype=None: np.ones_like(a, dtype=dtype)
  assert hasattr(jnp, 'quantile')


def make_images(rs, c):
  """gt, rendered rgb [patches, P, P, 3] and lossmult [patches, P, P, lm_c], float32-representable."""
  P, npatch = c['P'], c['patches']
  yy, xx = np.meshgrid(np.arange(P), np.arange(P), indexing='ij')
  gt = np.zeros((npatch, P, P, 3))
  resid = np.zeros((npatch, P, P, 3))
  for p in range(npatch):
    ph = rs.uniform(0, 2 * np.pi, 3)
    fr = rs.uniform(0.1, 0.6, (3, 2))
    for ch in range(3):
      gt[p, ..., ch] = 0.5 + 0.35 * np.sin(fr[ch, 0] * xx + fr[ch, 1] * yy + ph[ch])
    # smooth background error: small, with a per-patch level so that whole patches fall on either side of a mid threshold
    level = 10 ** rs.uniform(-2.6, -1.2)
    resid[p] = level * rs.standard_normal((P, P, 3)) * (0.6 + 0.4 * np.sin(0.4 * xx + rs.uniform(0, 6)))[..., None]
    kind = rs.randint(4)
    for _ in range(kind):                                         # blobs of large error (a distractor covering part of the patch)
      cy, cx, rad = rs.uniform(0, P), rs.uniform(0, P), rs.uniform(0.1, 0.6) * P
      blob = ((yy - cy) ** 2 + (xx - cx) ** 2) < rad ** 2
      resid[p][blob] += rs.uniform(0.2, 0.5, 3) * rs.choice([-1, 1], 3)
      specks = blob & (rs.uniform(size=(P, P)) < 0.08)            # clean specks inside the blob
      resid[p][specks] = level * 0.1 * rs.standard_normal((int(specks.sum()), 3))
    salt = rs.uniform(size=(P, P)) < 0.03                         # isolated bad pixels on the background
    resid[p][salt] += rs.uniform(0.2, 0.4, (int(salt.sum()), 3))
  gt = gt.astype(np.float32)
  rgb = (gt.astype(np.float64) + resid).astype(np.float32)
  lm = rs.choice([0.25, 0.5, 1.0, 2.0, 4.0], (npatch, P, P, c['lm_c'])).astype(np.float32)   # multiscale weights
  lm[rs.uniform(size=lm.shape) < 0.05] = 0.0                                                  # ... and masked-out rays
  return gt, rgb, lm


def try_case(name, c, seed, robustnerf, ref):
  rs = np.random.RandomState(seed)
  P, n, npatch = c['P'], c['P'] ** 2, c['patches']
  gt, rgb, lm = make_images(rs, c)
  errors = (rgb.astype(np.float64) - gt.astype(np.float64)) ** 2            # train_utils.py:86
  err_pp = errors.mean(-1).reshape(-1)
  thr = c['thr']
  if thr == 'mid':
    thr = float(np.float32(np.quantile(err_pp, rs.uniform(0.45, 0.7))))
  if not np.all(np.abs(err_pp - thr) > 1e-5 * thr):
    return None
  cfg = types.SimpleNamespace(robustnerf_inlier_quantile=c['qi'], enable_robustnerf_loss=c['enable'], patch_size=P,
                              robustnerf_inner_patch_size=c['inner'], robustnerf_smoothed_filter_size=c['f'],
                              robustnerf_smoothed_inlier_quantile=c['qs'], robustnerf_inner_patch_inlier_quantile=c['qp'])
  mask, stats = robustnerf.robustnerf_mask(errors, thr, cfg)
  mask = np.asarray(mask, np.float64).reshape(-1)
  B_valid = npatch * n
  B = c['B'] or B_valid
  kw = dict(B_valid=B_valid, patch_size=P, inner_patch_size=c['inner'], filter_size=c['f'], smoothed_inlier_quantile=c['qs'],
            inner_patch_inlier_quantile=c['qp'], enable=c['enable'])

  def pad(x):                                                                # the batch as the kernels see it: [B, c]
    x = x.reshape(B_valid, -1)
    return np.concatenate([x, np.repeat(x[-1:], B - B_valid, 0)], 0)

  rgb_b, gt_b, lm_b = pad(rgb), pad(gt), pad(lm)
  if c['enable']:
    own = ref.robustnerf_mask_f64(rgb_b, gt_b, thr, **kw)
    if np.any(np.abs(own['box_votes'] / c['f'] ** 2 - (1 - c['qs'])) < 1e-9):
      return None
    if np.any(np.abs(own['patch_votes'] / n - (1 - c['qp'])) < 1e-9):
      return None
    if c['thr'] == 'mid':
      # every criterion decides some pixel alone, and some pixels are masked out
      pr = own['parts']
      # (a 1 x 1 window repeats the pixel's own test: only the patch vote can add pixels there)
      alone = [pr[k] & ~np.any([pr[j] for j in pr if j != k], 0) for k in pr if c['f'] > 1 or k == 'patch']
      if not (all(a.any() for a in alone) and (mask == 0).any()):
        return None
  mask_b = np.concatenate([mask, np.zeros(B - B_valid)])
  denom = float(np.broadcast_to(lm.astype(np.float64), errors.shape).sum())
  mse = float((lm.astype(np.float64) * errors).sum() / denom)                # train_utils.py:87-88
  st = np.array([float(stats.get(k, 0.0)) for k in ('is_inlier_loss', 'has_inlier_neighbors', 'is_inlier_patch', 'mask')])
  return {
      'rgb': rgb_b, 'gt': gt_b, 'lossmult': lm_b, 'threshold': np.float64(thr),
      'params': np.array([P, c['inner'], c['f'], B_valid, int(c['enable'])], np.int64),
      'quantiles': np.array([c['qs'], c['qp'], c['qi']], np.float64),
      'mask': mask_b, 'lossmult_masked': lm_b.astype(np.float64) * mask_b[:, None], 'stats': st, 'mse': np.float64(mse),
      'next_threshold': np.float64(stats['loss_threshold']), 'seed': np.int64(seed),
  }


def write_gin_bindings():
  import json
  from multinerf_amd import configs, gin  # noqa: F401  (importing configs registers every configurable)
  gin.clear_config()
  gin.parse_config_file(os.path.join(make_golden.REF, 'configs', '360_robustnerf.gin'))
  out = {'360_robustnerf': {t: {a: repr(v) for a, v in b.items()} for t, b in gin._BINDINGS.items()}}
  gin.clear_config()
  with open(OUT_GIN, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
  print(f'wrote {OUT_GIN}')


def main():
  write_gin_bindings()
  jax = make_golden.install_jax_standin()
  install_missing(jax)
  sys.path.insert(0, make_golden.REF)
  from internal import robustnerf
  from tests import robustnerf_ref as ref
  out = {}
  for k, (name, c) in enumerate(CASES.items()):
    for seed in range(1000 * (k + 1), 1000 * (k + 1) + 200):
      g = try_case(name, c, seed, robustnerf, ref)
      if g is not None:
        break
    assert g is not None, f'{name}: no seed keeps every pixel clear of the threshold and every vote off its tie'
    for key, v in g.items():
      out[f'{name}/{key}'] = v
    print(f"{name}: seed {int(g['seed'])}, threshold {float(g['threshold']):.6g}, means {np.round(g['stats'], 4)}, "
          f"next threshold {float(g['next_threshold']):.6g}")
  np.savez_compressed(OUT, **out)
  print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes)')


if __name__ == '__main__':
  main()
