"""Functions for processing and scoring images (reference internal/image.py, and the per-image part of eval.py:118-163).

Images are device tensors and stay there: the sums behind PSNR, SSIM and the colour correction's normal equations are
HIP kernels (csrc/metrics.hip, through multinerf_amd.ops); what crosses to the host is scalars, and per colour-correction
iteration three 10 x 10 systems.  There is no CPU fallback: a host tensor is refused.
"""

import math

import numpy as np
import torch

from multinerf_amd import ops

_F32_EPS = float(np.finfo(np.float32).eps)


def mse_to_psnr(mse):
  """Compute PSNR given an MSE (we assume the maximum pixel value is 1)."""
  if isinstance(mse, torch.Tensor):
    return -10. / math.log(10.) * torch.log(mse)
  return -10. / math.log(10.) * math.log(mse) if mse > 0 else math.inf


def psnr_to_mse(psnr):
  """Compute MSE given a PSNR (we assume the maximum pixel value is 1)."""
  if isinstance(psnr, torch.Tensor):
    return torch.exp(-0.1 * math.log(10.) * psnr)
  return math.exp(-0.1 * math.log(10.) * psnr)


def ssim_to_dssim(ssim):
  """Compute DSSIM given an SSIM."""
  return (1 - ssim) / 2


def dssim_to_ssim(dssim):
  """Compute DSSIM given an SSIM."""
  return 1 - 2 * dssim


def linear_to_srgb(linear, eps=None):
  """Assumes `linear` is in [0, 1], see https://en.wikipedia.org/wiki/SRGB."""
  if eps is None:
    eps = _F32_EPS
  srgb0 = 323 / 25 * linear
  srgb1 = (211 * torch.clamp(linear, min=eps)**(5 / 12) - 11) / 200
  return torch.where(linear <= 0.0031308, srgb0, srgb1)


def srgb_to_linear(srgb, eps=None):
  """Assumes `srgb` is in [0, 1], see https://en.wikipedia.org/wiki/SRGB."""
  if eps is None:
    eps = _F32_EPS
  linear0 = 25 / 323 * srgb
  linear1 = torch.clamp((200 * srgb + 11) / 211, min=eps)**(12 / 5)
  return torch.where(srgb <= 0.04045, linear0, linear1)


def downsample(img, factor):
  """Area downsample img (factor must evenly divide img height and width)."""
  sh = tuple(img.shape)
  if not (sh[0] % factor == 0 and sh[1] % factor == 0):
    raise ValueError(f'Downsampling factor {factor} does not evenly divide image shape {sh[:2]}')
  img = img.reshape((sh[0] // factor, factor, sh[1] // factor, factor) + sh[2:])
  return img.mean((1, 3))


def _ingest_host(x, n, mode, c_out):
  """mnr_image_ingest's arithmetic in NumPy float32 (what the loaders did on the host): (out, alpha or None)."""
  u8 = x.dtype == np.uint8
  if n > 1:                                                   # image.downsample: the mean over n x n blocks
    acc = np.zeros((x.shape[0], x.shape[1] // n, x.shape[2] // n, x.shape[3]), np.uint32 if u8 else np.float64)
    for dy in range(n):                                       # row by row, the order the kernel adds in
      for dx in range(n):
        acc += x[:, dy::n, dx::n]
    m = acc.astype(np.float32) / np.float32(n * n) if u8 else (acc / np.float64(n * n)).astype(np.float32)
  else:
    m = x.astype(np.float32)
  if mode == 'normals':
    return m[..., :3] * np.float32(2.) / np.float32(255.) - np.float32(1.), None
  v = m / np.float32(255.) if u8 else m
  if mode == 'white_bg':
    rgb, alpha = v[..., :3], v[..., 3:]
    return rgb * alpha + (np.float32(1.) - alpha), np.ascontiguousarray(alpha[..., 0])
  return np.ascontiguousarray(v[..., :c_out]), None


def ingest(pixels, factor=1, mode='plain', device='cuda', c_out=None):
  """The single place where loaders turn decoded pixels into the float32 images a dataset keeps on its device.

  pixels: [N,H,W,C] uint8 or float32, a NumPy array or a tensor.  The area downsample by `factor` (image.downsample), then by
  `mode`: 'plain' (uint8 `/ 255.`, float32 unchanged; the first `c_out` channels), 'white_bg' (RGBA composited over white,
  `rgb * alpha + (1. - alpha)`) or 'normals' (uint8 `x * 2. / 255. - 1.`), in the reference's float32 order.  A height or
  width that `factor` does not divide is cropped at the bottom / right first; the reference's image.downsample raises there.

  On a HIP device the stack is uploaded as it is (bytes stay bytes) and ops.image_ingest does the arithmetic; with
  device 'cpu' the same expressions are evaluated in NumPy float32 and give the same bits.  Returns the image tensor
  [N,h,w,c] on `device`, for 'white_bg' the pair (images, alpha [N,h,w])."""
  device = torch.device(device)
  n = max(int(factor), 1)
  x = pixels if isinstance(pixels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pixels))
  if x.dim() != 4 or x.dtype not in (torch.uint8, torch.float32):
    raise ValueError(f'ingest: needs [N,H,W,C] uint8 or float32 pixels, got {tuple(x.shape)} {x.dtype}')
  h, w = x.shape[1] // n * n, x.shape[2] // n * n
  if h == 0 or w == 0:
    raise ValueError(f'ingest: factor {n} is larger than the image {tuple(x.shape[1:3])}')
  x = x[:, :h, :w]
  if mode not in ('plain', 'white_bg', 'normals'):
    raise ValueError(f'ingest: unknown mode {mode!r}')
  if c_out is None:
    c_out = x.shape[3] if mode == 'plain' else 3
  if mode == 'white_bg' and x.shape[3] != 4:
    raise ValueError(f'ingest: mode \'white_bg\' needs RGBA pixels, got {x.shape[3]} channels')
  if mode == 'normals' and (x.dtype != torch.uint8 or x.shape[3] < 3):
    raise ValueError('ingest: mode \'normals\' needs uint8 pixels with at least 3 channels')
  if not 1 <= c_out <= x.shape[3]:
    raise ValueError(f'ingest: c_out = {c_out} must be between 1 and the {x.shape[3]} channels of the pixels')
  if device.type == 'cpu':
    out, alpha = _ingest_host(x.cpu().numpy(), n, mode, c_out)
    out = torch.from_numpy(np.ascontiguousarray(out))
    return out if mode != 'white_bg' else (out, torch.from_numpy(alpha))
  return ops.image_ingest(x.contiguous().to(device), n, mode, c_out, want_alpha=mode == 'white_bg')


def solve_warp(gram):
  """The [10,3] warp of one colour-correction iteration from the kernel's [3,65] sums: per channel
  numpy.linalg.lstsq(A^T A, A^T b) in float64.  lstsq and not solve: a grey image makes the system rank deficient, and
  the minimum-norm solution of the normal equations is the one lstsq on the [pixels, 10] system gives."""
  gram = np.asarray(gram, np.float64)
  iu = np.triu_indices(10)
  warp = np.empty((10, 3))
  for c in range(3):
    G = np.zeros((10, 10))
    G[iu] = gram[c, :55]
    G = G + np.triu(G, 1).T
    w = np.linalg.lstsq(G, gram[c, 55:], rcond=None)[0]
    assert np.all(np.isfinite(w))
    warp[:, c] = w
  return warp


def color_correct(img, ref, num_iters=5, eps=0.5 / 255):
  """Warp `img` to match the colors in `ref_img` (image.py:81-124): a quadratic colour transform fitted by least squares
  over the unsaturated pixels, five times.  Device tensors of any float type; the result is float64, the precision the
  reference's eval.py:118-123 runs it in."""
  if img.shape[-1] != ref.shape[-1]:
    raise ValueError(f'img\'s {img.shape[-1]} and ref\'s {ref.shape[-1]} channels must match')
  if img.shape[-1] != 3 or img.shape != ref.shape:
    raise ValueError(f'color_correct: needs two RGB images of one shape, got {tuple(img.shape)} and {tuple(ref.shape)}')
  if not (ops._on_device(img) and ops._on_device(ref)):
    raise ValueError('color_correct: img and ref must be device tensors (the HIP path has no CPU fallback)')
  img_mat = img.reshape(-1, 3).to(torch.float64).contiguous()
  if img_mat.data_ptr() == img.data_ptr():
    img_mat = img_mat.clone()                                   # (updated in place below)
  ref_mat = ref.reshape(-1, 3).to(torch.float64).contiguous()
  mask0 = torch.empty(img_mat.shape, dtype=torch.uint8, device=img_mat.device)
  gram = torch.empty((3, 65), dtype=torch.float64, device=img_mat.device)
  for it in range(num_iters):
    ops.cc_gram(img_mat, ref_mat, mask0, eps, write_mask0=(it == 0), out=gram)
    warp = solve_warp(gram.cpu().numpy())
    ops.cc_apply(img_mat, warp, out=img_mat)
  return img_mat.reshape(img.shape)


class MetricHarness:
  """A helper class for evaluating several error metrics (image.py:127-141): PSNR and dm_pix.ssim.

  `quantize` and `crop` fold eval.py:134-143 into the kernels: the prediction is rounded to 8 bits (np.round) and both
  images are cropped by `crop` pixels at every border, by index arithmetic, before either metric is taken."""

  def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s, *, quantize=False, crop=0):
    """Evaluate the error between a predicted rgb image and the true image."""
    if rgb_pred.dim() != 3 or rgb_pred.shape != rgb_gt.shape:
      raise ValueError(f'MetricHarness: needs two [H,W,C] images of one shape, got {tuple(rgb_pred.shape)} and {tuple(rgb_gt.shape)}')
    pred = rgb_pred.contiguous()
    gt = rgb_gt.contiguous()
    if quantize or pred.dtype != torch.float32:             # SSIM takes the float32 image the statistics pass writes
      pred32 = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
      sq = ops.image_sqdiff(pred, gt, quantize=quantize, crop=crop, q_out=pred32)
    else:
      pred32 = pred
      sq = ops.image_sqdiff(pred, gt, crop=crop)
    gt32 = gt if gt.dtype == torch.float32 else gt.to(torch.float32)
    ssim = ops.ssim(pred32, gt32, crop=crop)
    h, w, c = pred.shape
    both = torch.cat([sq, ssim]).cpu()
    psnr = float(mse_to_psnr(float(both[0]) / ((h - 2 * crop) * (w - 2 * crop) * c)))
    return {
        name_fn('psnr'): psnr,
        name_fn('ssim'): float(both[1]),
    }


def quantize_u8(img):
  """The uint8 host image np.round(img * 255) of a device image in [0, 1]: what eval_quantize_metrics scores."""
  return np.clip(np.rint(img.detach().to(torch.float64).cpu().numpy() * 255.0), 0, 255).astype(np.uint8)


def evaluate_image(rendering, batch, config, metric_harness=None, postprocess_fn=None):
  """What the reference's eval.py:118-163 does with one rendered test image, in that order: colour-correct the rendering
  against the ground truth in float64, quantise both versions to 8 bits (Config.eval_quantize_metrics), crop the borders
  (Config.eval_crop_borders), PSNR + SSIM of each, then the disparity and normal metrics.

  postprocess_fn (RawNeRF: the dataset's metadata['postprocess_fn']) maps the rendering, its colour-corrected version and
  the ground truth from raw space to sRGB after the colour correction and before everything else (eval.py:130-132); the
  `color` / `color_cc` images returned are the post-processed ones.  With it, Config.eval_raw_affine_cc replaces the
  quadratic colour correction by raw_utils.match_images_affine.

  rendering: the dict of models.render_image ([H,W,...] device tensors); batch: the test batch (rgb, and disps / normals /
  alphas where the metrics need them).  Returns (metric, metric_cc, images_to_save); rendering['rgb_cc'] is added as the
  reference does.  images_to_save maps the reference's file stems (color, color_cc, distance_mean, distance_median,
  normals, acc) to device tensors."""
  if config.eval_raw_affine_cc and postprocess_fn is None:
    raise ValueError('Config.eval_raw_affine_cc = True is not supported: raw_utils.match_images_affine and the raw '
                     'post-processing need the DNG metadata of the RawNeRF loader')
  if metric_harness is None:
    metric_harness = MetricHarness()
  gt_rgb = batch.rgb[..., :3].to(torch.float64)                                      # eval.py:119-120
  rgb = rendering['rgb'].to(torch.float64)
  if config.eval_raw_affine_cc:                                                      # eval.py:63-66
    from multinerf_amd import raw_utils
    rendering['rgb_cc'] = raw_utils.match_images_affine(rgb, gt_rgb)
  else:
    rendering['rgb_cc'] = color_correct(rgb, gt_rgb)                                 # :123
  rgb_cc = rendering['rgb_cc']
  if postprocess_fn is not None:                                                     # :130-132
    rgb, rgb_cc, gt_rgb = postprocess_fn(rgb), postprocess_fn(rgb_cc), postprocess_fn(gt_rgb)
  quant, crop = bool(config.eval_quantize_metrics), int(config.eval_crop_borders)
  metric = metric_harness(rgb, gt_rgb, quantize=quant, crop=crop)                    # :134-145
  metric_cc = metric_harness(rgb_cc, gt_rgb, quantize=quant, crop=crop)
  n = rgb.shape[0] * rgb.shape[1]
  flat = lambda x, c=None: x.reshape((n,) if c is None else (n, c)).to(torch.float32).contiguous()
  if config.compute_disp_metrics:                                                    # :148-154
    if getattr(batch, 'disps', None) is None:
      raise ValueError('compute_disp_metrics needs batch.disps')
    for tag in ('mean', 'median'):
      key = f'distance_{tag}'
      if rendering.get(key) is not None:
        out = torch.zeros(1, dtype=torch.float32, device=rgb.device)
        ops.render_metrics(n, distance_mean=flat(rendering[key]), disps=flat(batch.disps), out_disp=out)
        metric[f'disparity_{tag}_mse'] = float(out.cpu()[0])
  if config.compute_normal_metrics:                                                  # :156-163
    if getattr(batch, 'normals', None) is None or getattr(batch, 'alphas', None) is None:
      raise ValueError('compute_normal_metrics needs batch.normals and batch.alphas')
    for key, val in list(rendering.items()):
      if key.startswith('normals') and val is not None:
        out = torch.zeros(1, dtype=torch.float32, device=rgb.device)
        ops.render_metrics(n, acc=flat(rendering['acc']), alphas=flat(batch.alphas), normals=flat(val, 3),
                           normals_gt=flat(batch.normals, 3), out_normal=out)        # (train_utils' weighted MAE kernel)
        metric[key + '_mae'] = float(out.cpu()[0])
  images = {'color': rendering['rgb'], 'color_cc': rendering['rgb_cc']} if postprocess_fn is None else \
      {'color': rgb, 'color_cc': rgb_cc}                                             # :171-188
  for key in ('distance_mean', 'distance_median', 'normals', 'acc'):
    if rendering.get(key) is not None:
      images[key] = rendering[key]
  return metric, metric_cc, images
