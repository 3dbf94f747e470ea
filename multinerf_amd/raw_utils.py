"""Functions for processing and loading raw image data (reference internal/raw_utils.py).

The per-pixel work runs on the device (csrc/raw.hip through multinerf_amd.ops): black / white level normalisation,
bilinear demosaic and area downsample in one kernel, the camera-to-sRGB post-processing in float64, an exact percentile
for the exposure levels, and the affine colour match of eval.py.  Images are device tensors and stay there; there is no
CPU fallback (a host tensor is refused).  EXIF handling is NumPy float64 on the host.

Mosaics come from `<name>.dng` through `rawpy` when `rawpy` can be imported.  Where it cannot, a `<name>.npy` file next
to `<name>.json` stands in for the DNG: a 2-D uint16 array holding what `rawpy.imread(f).raw_image` returns.
"""

import glob
import json
import os

import numpy as np
import torch

from multinerf_amd import ops


def _rawpy():
  try:
    import rawpy
    return rawpy
  except ImportError:
    return None


def _host_matrix(camtorgb):
  if isinstance(camtorgb, torch.Tensor):
    camtorgb = camtorgb.detach().cpu().numpy()
  camtorgb = np.asarray(camtorgb, np.float64)
  if camtorgb.shape != (3, 3):
    raise ValueError(f'camtorgb.shape is {camtorgb.shape}, expected (3, 3)')
  return camtorgb.reshape(-1)


def postprocess_raw(raw, camtorgb, exposure=None, want=None):
  """Converts demosaicked raw to sRGB with a minimal postprocessing pipeline (raw_utils.py:35-66).

  raw: [..., 3] float32 or float64 device tensor; camtorgb: [3, 3] (host); exposure: the colour value scaled to pure
  white, a float or a float64 device scalar; None "autoexposes" at the 97th percentile, on the device.  The arithmetic is
  float64; the result has the dtype of `raw`, or what `want` names ('f64', 'f32', 'u8', or a tuple of them)."""
  m = _host_matrix(camtorgb)
  raw = raw.contiguous()
  if exposure is None:
    exposure = ops.quantile_f64(ops.raw_postprocess(raw, m, linear_only=True), 97.)
  if want is None:
    want = 'f64' if raw.dtype == torch.float64 else 'f32'
  return ops.raw_postprocess(raw, m, exposure, want=(want,) if isinstance(want, str) else tuple(want))


def pixels_to_bayer_mask(pix_x, pix_y):
  """Computes binary RGB Bayer mask values from integer pixel coordinates (device tensors): red at (0, 0)."""
  x1, y1 = pix_x % 2 == 1, pix_y % 2 == 1
  r = ~x1 & ~y1
  g = x1 ^ y1
  b = x1 & y1
  return torch.stack([r, g, b], -1).to(torch.float32)


def bilinear_demosaic(bayer, xnp=None):
  """Converts Bayer data [H, W] (or [N, H, W]; RGGB, uint16 or float32, on the device) into a full RGB image using bilinear
  demosaicking (raw_utils.py:80-146, its wrap-around at the borders included).  `xnp` is accepted and ignored."""
  return ops.raw_demosaic(bayer.contiguous())


def load_raw_images(image_dir, image_names=None):
  """Loads raw images and their metadata from disk (raw_utils.py:152-191).

  Per image `<base>.json` (as `exiftool -json` writes it; element 0 is used) and the mosaic: `<base>.dng` through rawpy when
  that is installed, otherwise `<base>.npy`.  Returns (raws [N, H, W] uint16 on the host, exifs)."""
  if not os.path.exists(image_dir):
    raise ValueError(f'Raw image folder {image_dir} does not exist.')
  rawpy = _rawpy()

  def load_mosaic(base):
    if rawpy is not None and os.path.exists(base + '.dng'):
      with open(base + '.dng', 'rb') as f:
        return np.array(rawpy.imread(f).raw_image)
    if os.path.exists(base + '.npy'):
      raw = np.load(base + '.npy')
      if raw.ndim != 2 or raw.dtype != np.uint16:
        raise ValueError(f'{base}.npy must hold a 2-D uint16 mosaic, holds {raw.dtype} {raw.shape}')
      return raw
    raise ValueError(f'No raw mosaic for {base}: it needs {base}.dng and the rawpy package (rawpy '
                     f'{"is" if rawpy is not None else "is not"} installed), or {base}.npy, a 2-D uint16 array holding '
                     'what rawpy.imread(f).raw_image returns')

  def load_raw_exif(image_name):
    base = os.path.join(image_dir, os.path.splitext(image_name)[0])
    raw = load_mosaic(base)
    if not os.path.exists(base + '.json'):
      raise ValueError(f'No EXIF metadata {base}.json (written by `exiftool -json`)')
    with open(base + '.json', 'rb') as f:
      exif = json.load(f)[0]
    return raw, exif

  if image_names is None:
    ext = '.dng' if rawpy is not None and glob.glob(os.path.join(image_dir, '*.dng')) else '.npy'
    image_names = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(image_dir, '*' + ext)))]
  if not image_names:
    raise ValueError(f'No raw images in {image_dir}: it needs *.dng files and the rawpy package, or *.npy mosaics')
  raws, exifs = zip(*[load_raw_exif(x) for x in image_names])
  return np.stack(raws, axis=0), exifs


# Brightness percentiles to use for re-exposing and tonemapping raw images.
_PERCENTILE_LIST = (80, 90, 97, 99, 100)

# Relevant fields to extract from raw image EXIF metadata (the DNG specification 1.4.0.0).
_EXIF_KEYS = (
    'BlackLevel',  # Black level offset added to sensor measurements.
    'WhiteLevel',  # Maximum possible sensor measurement.
    'AsShotNeutral',  # RGB white balance coefficients.
    'ColorMatrix2',  # XYZ to camera color space conversion matrix.
    'NoiseProfile',  # Shot and read noise levels.
)

# Color conversion from reference illuminant XYZ to RGB color space.
# See http://www.brucelindbloom.com/index.html?Eqn_RGB_XYZ_Matrix.html.
_RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375],
                     [0.2126729, 0.7151522, 0.0721750],
                     [0.0193339, 0.1191920, 0.9503041]])


def process_exif(exifs):
  """Processes a list of raw image EXIF dicts (one per image, as loaded from `exiftool -json` files) into the metadata
  RawNeRF needs (raw_utils.py:215-270): levels, white balance, colour matrix, noise profile, 'ShutterSpeed' in seconds
  and the raw-to-sRGB matrices 'cam2rgb' [N, 3, 3].  NumPy float64."""
  meta = {}
  exif = exifs[0]
  for key in _EXIF_KEYS:
    exif_value = exif.get(key)
    if exif_value is None:
      continue
    if isinstance(exif_value, (int, float)):                 # a single number ...
      vals = [x[key] for x in exifs]
    elif isinstance(exif_value, str):                        # ... or a string of numbers with ' ' between
      vals = [[float(z) for z in x[key].split(' ')] for x in exifs]
    else:
      raise ValueError(f'EXIF field {key} is neither a number nor a string: {exif_value!r}')
    meta[key] = np.squeeze(np.array(vals))
  # Shutter speed is a special case, a string written like 1/N.
  meta['ShutterSpeed'] = np.fromiter((1. / float(x['ShutterSpeed'].split('/')[1]) for x in exifs), float)
  # cam space -> white balanced cam space ("camwb") -> XYZ space -> RGB space.
  whitebalance = meta['AsShotNeutral'].reshape(-1, 3)
  cam2camwb = np.array([np.diag(1. / x) for x in whitebalance])
  xyz2camwb = meta['ColorMatrix2'].reshape(-1, 3, 3)
  rgb2camwb = xyz2camwb @ _RGB2XYZ
  rgb2camwb /= rgb2camwb.sum(axis=-1, keepdims=True)         # rows normalised (simple-camera-pipeline)
  meta['cam2rgb'] = np.linalg.inv(rgb2camwb) @ cam2camwb
  return meta


def process_raw_capture(raws, meta, shutter_ratio, exposure_percentile, n_downsample, device):
  """The second half of load_raw_dataset (raw_utils.py:339-384) for mosaics [N, H, W] (host uint16 or float32) and the
  metadata of process_exif: exposure indices, the exposure levels of full-resolution image 0, the post-processing
  function, and the normalised, demosaicked, downsampled images [N, H/n, W/n, 3] float32 on `device`."""
  shutter_speeds = meta['ShutterSpeed']
  # Sort the shutter speeds from slowest (largest) to fastest (smallest): index 0 is the brightest image.
  unique_shutters = np.sort(np.unique(shutter_speeds))[::-1]
  exposure_idx = np.zeros_like(shutter_speeds, dtype=np.int32)
  for i, shutter in enumerate(unique_shutters):
    exposure_idx[shutter_speeds == shutter] = i
  meta['exposure_idx'] = exposure_idx
  meta['unique_shutters'] = unique_shutters
  meta['exposure_values'] = shutter_speeds / unique_shutters[0]

  raws = np.ascontiguousarray(raws)
  if raws.dtype not in (np.uint16, np.float32):
    raise ValueError(f'raw mosaics must be uint16 or float32, are {raws.dtype}')
  n = raws.shape[0]
  level = lambda k: torch.as_tensor(np.broadcast_to(np.asarray(meta[k], np.float64).reshape(-1), (n,)).copy()).to(device)
  black, white = level('BlackLevel'), level('WhiteLevel')
  mosaics = torch.as_tensor(raws).to(device)

  # The exposure level for gamma mapping: always based on full-resolution image 0.
  cam2rgb0 = meta['cam2rgb'][0]
  image0 = ops.raw_demosaic(mosaics[:1], black[:1], white[:1], shutter_ratio)
  image0_rgb = ops.raw_postprocess(image0, cam2rgb0.reshape(-1), linear_only=True)
  ps = (exposure_percentile,) + _PERCENTILE_LIST
  levels = torch.cat([ops.quantile_f64(image0_rgb, p) for p in ps]).cpu().numpy()
  exposure = float(levels[0])
  meta['exposure'] = exposure
  meta['exposure_levels'] = {p: float(v) for p, v in zip(_PERCENTILE_LIST, levels[1:])}
  del image0, image0_rgb
  # An explicit None auto-exposes every image at its own 97th percentile.
  meta['postprocess_fn'] = lambda z, x=exposure, **kw: postprocess_raw(z, cam2rgb0, x, **kw)

  images = ops.raw_demosaic(mosaics, black, white, shutter_ratio, n_downsample)
  return images, meta


def load_raw_dataset(split, data_dir, image_names, exposure_percentile, n_downsample, device='cuda'):
  """Loads and processes a set of RawNeRF input images (raw_utils.py:273-384), the special "test" scenes with a noiseless
  HDR+ ground truth frame (`hdrplus_test/merged.dng`, or `.npy` without rawpy) included.

  split: 'train' or 'test'.  Returns (images [N, H/n, W/n, 3] float32 on `device`, meta, testscene)."""
  image_dir = os.path.join(data_dir, 'raw')
  rawpy = _rawpy()
  testimg_base = os.path.join(data_dir, 'hdrplus_test', 'merged')
  testscene = (rawpy is not None and os.path.exists(testimg_base + '.dng')) or os.path.exists(testimg_base + '.npy')
  if testscene:
    # Test scenes have train/ and test/ split subdirectories inside raw/.
    image_dir = os.path.join(image_dir, split)
    if split == 'test':
      image_names = None                                     # COLMAP image names not valid for test split of test scene.
    else:
      image_names = image_names[1:]                          # The first COLMAP image is a copy of the test image.

  raws, exifs = load_raw_images(image_dir, image_names)
  meta = process_exif(exifs)

  if testscene and split == 'test':
    if rawpy is not None and os.path.exists(testimg_base + '.dng'):
      with open(testimg_base + '.dng', 'rb') as f:
        testraw = np.array(rawpy.imread(f).raw_image)
    else:
      testraw = np.load(testimg_base + '.npy')
    testraw = testraw.astype(np.float32) / 4.                # HDR+ output has 2 extra bits of fixed precision.
    shutter_ratio = meta['ShutterSpeed'][0] / meta['ShutterSpeed'][-1]      # fast : slow
    raws = testraw[None]
    meta = {k: meta[k][:1] for k in meta}                    # shares metadata with the first loaded image
  else:
    shutter_ratio = 1.

  images, meta = process_raw_capture(raws, meta, shutter_ratio, exposure_percentile, n_downsample, device)
  return images, meta, testscene


# XYZ (D65) -> linear sRGB, the inverse of _RGB2XYZ (same source): as ColorMatrix2 it makes cam2rgb the white balance alone.
_SYNTH_COLOR_MATRIX = '3.2404542 -1.5371385 -0.4985314 -0.9692660 1.8760108 0.0415560 0.0556434 -0.2040259 1.0572252'
_SYNTH_SHUTTERS = ('1/30', '1/60', '1/120')
_SYNTH_BLACK, _SYNTH_WHITE = 64, 1023


def synthesize_raw_capture(images, split, seed=0):
  """A raw capture of the procedural scene: images [N, H, W, 3] in [0, 1] (host) are 0.25 x the scene radiance in linear
  camera RGB, exposed with shutters 1/30, 1/60, 1/120 in turn ('test': 1/30), sampled through the RGGB pattern, with
  Gaussian noise of variance 1e-4 clean + 1e-6, and quantised to 10-bit digital numbers over a black level of 64.
  Returns (mosaics [N, H, W] uint16, exifs in exiftool's form); both go through the code that files go through."""
  images = np.asarray(images, np.float64)
  n, h, w, _ = images.shape
  if h % 2 or w % 2:
    raise ValueError(f'a Bayer mosaic has even height and width, got [{h}, {w}]')
  shutters = [_SYNTH_SHUTTERS[i % 3] if split == 'train' else _SYNTH_SHUTTERS[0] for i in range(n)]
  rel = np.array([float(_SYNTH_SHUTTERS[0].split('/')[1]) / float(s.split('/')[1]) for s in shutters])
  v = 0.25 * images * rel[:, None, None, None]
  ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
  channel = (ys % 2) + (xs % 2)                              # R at (0, 0), G at (0, 1) and (1, 0), B at (1, 1)
  clean = np.take_along_axis(v, np.broadcast_to(channel[None, ..., None], (n, h, w, 1)), -1)[..., 0]
  rng = np.random.default_rng([int(seed), 0 if split == 'train' else 1])
  noisy = clean + rng.standard_normal(clean.shape) * np.sqrt(1e-4 * clean + 1e-6)
  dn = np.clip(np.rint(_SYNTH_BLACK + (_SYNTH_WHITE - _SYNTH_BLACK) * noisy), 0, _SYNTH_WHITE).astype(np.uint16)
  exifs = [dict(BlackLevel=_SYNTH_BLACK, WhiteLevel=_SYNTH_WHITE, AsShotNeutral='1 1 1', ColorMatrix2=_SYNTH_COLOR_MATRIX,
                NoiseProfile='0.0001 1e-06', ShutterSpeed=s) for s in shutters]
  return dn, exifs


def best_fit_affine(x, y, axis=(0, 1)):
  """Computes best fit a, b such that a * x + b = y, in a least square sense, per channel over the image axes
  (raw_utils.py:387-396): x, y [..., 3] float64 device tensors; the sums are taken on the device, a and b [3] are NumPy."""
  if tuple(axis) != tuple(range(x.dim() - 1)):
    raise ValueError(f'best_fit_affine: axis {axis} must name every axis but the channels')
  sums = ops.affine_sums(y.contiguous(), x.contiguous()).cpu().numpy()      # rows: x, y, x y, x x
  x_m, y_m, xy_m, xx_m = sums / (x.numel() // 3)
  a = (xy_m - x_m * y_m) / (xx_m - x_m * x_m)                # slope a = Cov(x, y) / Cov(x, x)
  b = y_m - a * x_m
  return a, b


def match_images_affine(est, gt, axis=(0, 1)):
  """Computes affine best fit of gt->est, then maps est back to match gt (raw_utils.py:399-406).  Device tensors of any
  float type; the result is float64."""
  if est.shape != gt.shape or est.shape[-1] != 3:
    raise ValueError(f'match_images_affine: needs two RGB images of one shape, got {tuple(est.shape)} and {tuple(gt.shape)}')
  if not (ops._on_device(est) and ops._on_device(gt)):
    raise ValueError('match_images_affine: est and gt must be device tensors (the HIP path has no CPU fallback)')
  est64 = est.to(torch.float64).contiguous()
  gt64 = gt.to(torch.float64).contiguous()
  a, b = best_fit_affine(gt64, est64, axis=axis)             # gt->est: robust, since `est` may be very noisy
  return ops.affine_apply(est64, a, b)
