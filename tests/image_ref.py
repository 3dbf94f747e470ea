"""NumPy float64 restatements for the evaluation metrics (test infrastructure).

`ssim` restates dm_pix.ssim from its definition (dm_pix is not installable here): Gaussian window normalised to sum 1,
applied separably per channel with VALID padding; sigma00 / sigma11 clamped at float32_eps^2, sigma01 limited to
sqrt(sigma00 sigma11).  tests/golden/make_golden_image.py installs it as the stub `dm_pix.ssim` under the reference's own
MetricHarness; tests/test_image_cpu.py cross-checks it against an independent scipy formulation.

`color_correct` restates the reference's internal/image.py:81-124 step by step (lstsq on the masked [N, 10] system) and
can report its iterates; `color_correct_gram` is the form the device code uses (per-channel 10 x 10 normal equations
solved by lstsq), with the sums taken here in NumPy.
"""

import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)


def gaussian_window(filter_size=11, filter_sigma=1.5):
  x = (np.arange(filter_size, dtype=np.float64) - filter_size // 2) / filter_sigma
  w = np.exp(-0.5 * x * x)
  return w / w.sum()


def _filt(z, w):
  """VALID separable correlation of [H, W, C] with the window along both image axes."""
  f = len(w)
  H, W = z.shape[:2]
  h = sum(w[k] * z[:, k:W - f + 1 + k] for k in range(f))
  return sum(w[k] * h[k:H - f + 1 + k] for k in range(f))


def ssim(a, b, *, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False, **unused):
  a = np.asarray(a, np.float64)
  b = np.asarray(b, np.float64)
  w = gaussian_window(filter_size, filter_sigma)
  mu0, mu1 = _filt(a, w), _filt(b, w)
  mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
  sigma00 = _filt(a * a, w) - mu00
  sigma11 = _filt(b * b, w) - mu11
  sigma01 = _filt(a * b, w) - mu01
  eps = F32_EPS**2
  sigma00 = np.maximum(eps, sigma00)
  sigma11 = np.maximum(eps, sigma11)
  sigma01 = np.sign(sigma01) * np.minimum(np.sqrt(sigma00 * sigma11), np.abs(sigma01))
  c1, c2 = (k1 * max_val)**2, (k2 * max_val)**2
  numer = (2 * mu01 + c1) * (2 * sigma01 + c2)
  denom = (mu00 + mu11 + c1) * (sigma00 + sigma11 + c2)
  ssim_map = numer / denom
  value = float(np.mean(ssim_map))
  return (value, ssim_map) if return_map else value


def mse_to_psnr(mse):
  with np.errstate(divide='ignore'):                           # identical images: inf, as the reference gives
    return float(-10. / np.log(10.) * np.log(mse))


def metric_harness(pred, gt, *, quantize=False, crop=0, cast_f32=False):
  """eval.py:134-146: quantise the prediction, crop both, PSNR and SSIM.  cast_f32: SSIM takes the float32 roundings of
  its inputs (what jax does with the float64 arrays it is handed, and what the device code does)."""
  pred = np.asarray(pred, np.float64)
  gt = np.asarray(gt, np.float64)
  if quantize:
    pred = np.round(pred * 255) / 255
  if crop > 0:
    pred, gt = pred[crop:-crop, crop:-crop], gt[crop:-crop, crop:-crop]
  to = (lambda z: z.astype(np.float32).astype(np.float64)) if cast_f32 else (lambda z: z)
  return {'psnr': mse_to_psnr(((pred - gt)**2).mean()), 'ssim': ssim(to(pred), to(gt))}


def features(img_mat):
  """[N, 10]: r r, r g, r b, g g, g b, b b, r, g, b, 1 (image.py:98-103)."""
  cols = [img_mat[:, c:c + 1] * img_mat[:, c:] for c in range(3)]
  return np.concatenate(cols + [img_mat, np.ones_like(img_mat[:, :1])], axis=-1)


def unclipped(z, eps):
  return (z >= eps) & (z <= 1 - eps)


def color_correct(img, ref, num_iters=5, eps=0.5 / 255, trace=None):
  """image.py:81-124 in float64.  trace (a list) receives per iteration (img_mat before the solve, the three masks)."""
  img_mat = np.asarray(img, np.float64).reshape(-1, 3)
  ref_mat = np.asarray(ref, np.float64).reshape(-1, 3)
  mask0 = unclipped(img_mat, eps)
  for _ in range(num_iters):
    a_mat = features(img_mat)
    warp = []
    if trace is not None:
      trace.append((img_mat.copy(), mask0, unclipped(img_mat, eps), unclipped(ref_mat, eps)))
    for c in range(3):
      b = ref_mat[:, c]
      mask = mask0[:, c] & unclipped(img_mat[:, c], eps) & unclipped(b, eps)
      w = np.linalg.lstsq(np.where(mask[:, None], a_mat, 0), np.where(mask, b, 0), rcond=-1)[0]
      warp.append(w)
    img_mat = np.clip(a_mat @ np.stack(warp, axis=-1), 0, 1)
  return img_mat.reshape(np.shape(img))


def gram_sums(img_mat, ref_mat, mask0, eps):
  """[3, 65]: per channel the upper triangle of A^T A (row-major) and A^T b over the unmasked rows."""
  a_mat = features(img_mat)
  iu = np.triu_indices(10)
  out = np.zeros((3, 65))
  for c in range(3):
    mask = mask0[:, c] & unclipped(img_mat[:, c], eps) & unclipped(ref_mat[:, c], eps)
    am = a_mat[mask]
    out[c, :55] = (am.T @ am)[iu]
    out[c, 55:] = am.T @ ref_mat[mask, c]
  return out


def color_correct_gram(img, ref, solve_warp, num_iters=5, eps=0.5 / 255):
  """The device form on the host: normal equations per channel, `solve_warp` ([3,65] -> [10,3]) from the package."""
  img_mat = np.asarray(img, np.float64).reshape(-1, 3)
  ref_mat = np.asarray(ref, np.float64).reshape(-1, 3)
  mask0 = unclipped(img_mat, eps)
  for _ in range(num_iters):
    warp = solve_warp(gram_sums(img_mat, ref_mat, mask0, eps))
    img_mat = np.clip(features(img_mat) @ warp, 0, 1)
  return img_mat.reshape(np.shape(img))
