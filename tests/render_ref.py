"""NumPy float64 restatements for the visualisation kernels and the spherical camera (test infrastructure).

Each function restates, from its definition, what one entry of csrc/vis.hip (or mnr_spherical_rays) computes, on float64
copies of the float32 inputs the kernels get; tests/golden/make_golden_render.py records the reference's own outputs, and
tests/test_render_cpu.py cross-checks these restatements against those records, so the GPU tests can use either.
`host_colourise` is the host path of the reference's render.py:86-93 (NumPy, table lookup), the baseline the device
colourisation is timed against in profiles/render_path.md.
"""

import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)

CURVES = {
    None: lambda x: x,
    'identity': lambda x: x,
    'log': lambda x: np.log(x + F32_EPS),
    'neg_log': lambda x: -np.log(x + F32_EPS),
    'ln': np.log,
}


def weighted_percentile(x, w, ps):
  """vis.py:22-30 with the clamping gather jax documents for an out-of-range index (the depth triplet has 3 values per
  weight): stable argsort, cumsum, np.interp, all in float64."""
  x = np.asarray(x, np.float64).reshape(-1)
  w = np.asarray(w, np.float64).reshape(-1)
  order = np.argsort(x, kind='stable')
  x, w = x[order], w[np.minimum(order, len(w) - 1)]
  acc = np.cumsum(w)
  return np.interp(np.array(ps, np.float64) * (acc[-1] / 100), acc, x)


def checker(H, W, dark=0.8, light=1.0, width=8):
  mask = np.logical_xor((np.arange(H) % (2 * width) // width)[:, None], (np.arange(W) % (2 * width) // width)[None, :])
  return np.where(mask, light, dark)


def matte(vis, acc, dark=0.8, light=1.0, width=8):
  """vis.py:39-45."""
  vis, acc = np.asarray(vis, np.float64), np.asarray(acc, np.float64)
  bg = checker(acc.shape[0], acc.shape[1], dark, light, width)
  return vis * acc[:, :, None] + (bg * (1 - acc))[:, :, None]


def preop(name, x=None, origins=None, directions=None, distance=None):
  """The pre-ops of mnr_vis_matte (vis.py:255, :258, :185 + :111)."""
  if name == 'coord_mod':
    coords = np.asarray(origins, np.float64)
    if directions is not None:
      coords = coords + np.asarray(directions, np.float64) * np.asarray(distance, np.float64)[:, :, None]
    return np.mod(coords + 1, 2) / 2
  x = np.asarray(x, np.float64)
  return {None: x, 'half': x / 2 + 0.5, 'tanh': np.tanh(x)}[name]


def normalise(value, lo, hi, curve=None, modulus=None):
  """vis.py:86-94: the value in [0, 1] that goes into the colour map."""
  fn = CURVES[curve]
  with np.errstate(divide='ignore', invalid='ignore'):
    value = fn(np.asarray(value, np.float64))
    if modulus:
      return np.mod(value, modulus) / modulus
    lo, hi = fn(np.float64(lo)), fn(np.float64(hi))
    return np.nan_to_num(np.clip((value - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1))


def lut_index(v, n):
  """matplotlib's entry for a float in [0, 1]: trunc(v n), v = 1 in the last entry."""
  return np.minimum((v * n).astype(np.int64), n - 1)


def visualize_cmap_pixels(value, lo, hi, curve=None, modulus=None, lut=None, acc=None, dark=0.8, light=1.0, width=8):
  """The per-pixel part of vis.visualize_cmap with given bounds -> (image, LUT indices or None)."""
  v = normalise(value, lo, hi, curve, modulus)
  idx = None
  if lut is not None:
    if v.ndim == 3:
      v = v[..., 0]
    idx = lut_index(v, len(lut))
    col = np.asarray(lut, np.float64)[idx]
  else:
    col = v
  if acc is not None:
    col = matte(col, acc, dark, light, width)
  return col, idx


def spherical_rays(camtoworld, height, width):
  """camera_utils.py:724-751 in float64 -> (origins, directions, radii [H,W,1])."""
  c2w = np.asarray(camtoworld, np.float64)
  theta, phi = np.meshgrid(np.linspace(0, 2 * np.pi, width + 1), np.linspace(0, np.pi, height + 1), indexing='xy')
  d = np.stack([-np.sin(phi) * np.sin(theta), np.cos(phi), np.sin(phi) * np.cos(theta)], -1)
  d = np.matmul(c2w[:3, :3], d[..., None])[..., 0]
  dy = np.diff(d[:, :-1], axis=0)
  dx = np.diff(d[:-1, :], axis=1)
  d = d[:-1, :-1]
  radii = (0.5 * (np.linalg.norm(dx, axis=-1) + np.linalg.norm(dy, axis=-1)))[..., None] * 2 / np.sqrt(12)
  return np.broadcast_to(c2w[:3, -1], d.shape), d, radii


def host_colourise(img, lo, hi, lut, curve_fn=np.log):
  """render.py:88-93 on the host: curve, normalise between curve(lo) and curve(hi) (already curved here), colour map,
  8 bits.  `lut` [n,3] float64 stands for cm.get_cmap('turbo')."""
  with np.errstate(divide='ignore', invalid='ignore'):
    img = curve_fn(img)
    img = np.clip((img - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1)
  img = lut[lut_index(np.nan_to_num(img), len(lut))]
  return (np.clip(np.nan_to_num(img), 0., 1.) * 255.).astype(np.uint8)


def ulp32(x):
  """One float32 unit in the last place at |x| (float64 array)."""
  return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
