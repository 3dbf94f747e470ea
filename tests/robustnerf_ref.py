"""Float64 restatement of the RobustNeRF mask (reference internal/robustnerf.py:23-115) for the tests, written from the
paper's three criteria and NOT from the kernel: plain NumPy loops over the patches, votes counted in integers.

tests/test_robustnerf_cpu.py holds it to tests/golden/robustnerf.npz (the reference's own code on the NumPy stand-in);
the composed GPU tests then use it on the renderings of a real training step, where no recorded fixture can exist.
"""

import numpy as np

STAT_NAMES = ('is_inlier_loss', 'has_inlier_neighbors', 'is_inlier_patch', 'mask')


def per_pixel_error(rgb, gt):
  """mean_c (rgb - gt)^2 in float64, [B]."""
  d = np.asarray(rgb, np.float64) - np.asarray(gt, np.float64)
  return (d * d).mean(-1)


def robustnerf_mask_f64(rgb, gt, loss_threshold, *, B_valid, patch_size, inner_patch_size, filter_size,
                        smoothed_inlier_quantile, inner_patch_inlier_quantile, enable=True):
  """-> dict(mask [B] (0 behind B_valid), err [B_valid], stats {name: mean}, box_votes [B_valid] ints, patch_votes [patches]
  ints): the last two let a fixture generator prove that no vote sits on a tie."""
  rgb, gt = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
  B, P, f = rgb.shape[0], int(patch_size), int(filter_size)
  n = P * P
  assert B_valid % n == 0 and inner_patch_size <= P
  npatch = B_valid // n
  err = per_pixel_error(rgb[:B_valid], gt[:B_valid])
  mask = np.zeros(B)
  if not enable:
    mask[:B_valid] = 1.0
    return dict(mask=mask, err=err, stats={'mask': 1.0}, box_votes=None, patch_votes=None)
  inl = (err < float(loss_threshold)).reshape(npatch, P, P)
  h = f // 2
  padded = np.zeros((npatch, P + 2 * h, P + 2 * h), np.int64)
  padded[:, h:h + P, h:h + P] = inl
  votes = np.zeros((npatch, P, P), np.int64)
  for dy in range(f):
    for dx in range(f):
      votes += padded[:, dy:dy + P, dx:dx + P]
  has = votes / (f * f) > 1 - smoothed_inlier_quantile
  pixel = has | inl
  patch_votes = pixel.reshape(npatch, n).sum(-1)
  patch_in = patch_votes / n > 1 - inner_patch_inlier_quantile
  lo = (P - inner_patch_size) // 2
  rect = np.zeros((P, P), bool)
  rect[lo:lo + inner_patch_size, lo:lo + inner_patch_size] = True
  inner = patch_in[:, None, None] & rect[None]
  m = inner | pixel
  mask[:B_valid] = m.reshape(-1)
  stats = {'is_inlier_loss': inl.mean(), 'has_inlier_neighbors': has.mean(), 'is_inlier_patch': inner.mean(), 'mask': m.mean()}
  return dict(mask=mask, err=err, stats=stats, box_votes=votes.reshape(-1), patch_votes=patch_votes,
              parts=dict(loss=inl.reshape(-1), neighbors=has.reshape(-1), patch=inner.reshape(-1)))


def weighted_mse(rgb, gt, lossmult, B_valid):
  """train_utils.py:86-88 for one level: sum(lossmult * (rgb - gt)^2) / sum(lossmult), lossmult broadcast to [B,3]."""
  d = np.asarray(rgb, np.float64)[:B_valid] - np.asarray(gt, np.float64)[:B_valid]
  lm = np.broadcast_to(np.asarray(lossmult, np.float64)[:B_valid], d.shape)
  return float((lm * d * d).sum() / lm.sum())
