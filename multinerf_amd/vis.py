"""Helper functions for visualizing things (reference internal/vis.py), on the device.

A rendering is a dict of device tensors (models.render_image) and stays there: the weighted percentile, the colour map
with its normalisation and curve, and the checker matte are HIP kernels (csrc/vis.hip, through multinerf_amd.ops); the
order the percentile needs comes from torch.sort, the ray panels (visualize_rays, a few rays per image) are composed
from torch ops on the device.  Nothing is read back to the host.  There is no CPU fallback: a host tensor is refused.

Differences from the reference's signatures, both forced by the kernels taking tables instead of Python callables:
  * `curve_fn` is one of CURVE_IDENTITY, CURVE_LOG, CURVE_NEG_LOG (x, log(x + eps32), -log(x + eps32)) or their names
    'identity' / 'log' / 'neg_log'; another callable is refused.
  * `colormap` is a name (looked up in matplotlib, imported lazily, sampled once into a cached device table), a
    matplotlib colormap, or an [n,3] array / tensor; a value v in [0, 1] takes entry min(trunc(v n), n - 1), which is
    what a matplotlib colormap returns for a float.
"""

import numpy as np
import torch

from multinerf_amd import ops

_F32_EPS = float(np.finfo(np.float32).eps)


class _Curve:
  """A curve the colour-map kernel knows by id; callable on tensors for use outside it."""

  def __init__(self, name, fn):
    self.name, self._fn = name, fn

  def __call__(self, x):
    return self._fn(x)

  def __repr__(self):
    return f'vis.CURVE_{self.name.upper()}'


CURVE_IDENTITY = _Curve('identity', lambda x: x)
CURVE_LOG = _Curve('log', lambda x: torch.log(x + _F32_EPS))
CURVE_NEG_LOG = _Curve('neg_log', lambda x: -torch.log(x + _F32_EPS))
_CURVES = {c.name: c for c in (CURVE_IDENTITY, CURVE_LOG, CURVE_NEG_LOG)}


def _curve_name(curve_fn):
  if curve_fn is None:
    return 'identity'
  if isinstance(curve_fn, _Curve):
    return curve_fn.name
  if isinstance(curve_fn, str) and curve_fn in _CURVES:
    return curve_fn
  raise ValueError(f'curve_fn must be one of vis.CURVE_IDENTITY / CURVE_LOG / CURVE_NEG_LOG or {sorted(_CURVES)}, got {curve_fn!r} '
                   '(the colour-map kernel applies the curve itself; there is no Python path)')


_LUT_CACHE = {}


def colormap_lut(colormap, device):
  """The [n,3] float32 device table of a colormap: a name (matplotlib.colormaps[name], imported here and sampled once per
  name and device), a matplotlib colormap object, or an [n,3] array / tensor."""
  device = torch.device(device)
  if isinstance(colormap, torch.Tensor):
    lut = colormap.to(device=device, dtype=torch.float32)
  elif isinstance(colormap, str):
    key = (colormap, str(device))
    if key not in _LUT_CACHE:
      import matplotlib
      _LUT_CACHE[key] = colormap_lut(matplotlib.colormaps[colormap], device)
    return _LUT_CACHE[key]
  elif callable(colormap) and hasattr(colormap, 'N'):
    lut = torch.as_tensor(np.asarray(colormap(np.arange(colormap.N)))[:, :3].astype(np.float32)).to(device)
  else:
    lut = torch.as_tensor(np.asarray(colormap, dtype=np.float32)).to(device)
  if lut.dim() != 2 or lut.shape[1] < 3:
    raise ValueError(f'a colormap table must be [n,3], got {tuple(lut.shape)}')
  return lut[:, :3].contiguous()


def _f32(x):
  return x.to(torch.float32).contiguous()


def weighted_percentile(x, w, ps, assume_sorted=False):
  """Compute the weighted percentile(s) of a single vector (vis.py:22-30): a float32 device tensor [len(ps)]."""
  return ops.weighted_percentile(_f32(x), _f32(w), ps, assume_sorted=assume_sorted)


def sinebow(h):
  """A cyclic and uniform colormap, see http://basecase.org/env/on-rainbows."""
  f = lambda x: torch.sin(np.pi * x)**2
  return torch.stack([f(3 / 6 - h), f(5 / 6 - h), f(7 / 6 - h)], -1)


def matte(vis, acc, dark=0.8, light=1.0, width=8):
  """Set non-accumulated pixels to a Photoshop-esque checker pattern."""
  return ops.vis_matte(_f32(vis), _f32(acc), dark=dark, light=light, width=width)


def visualize_cmap(value, weight, colormap, lo=None, hi=None, percentile=99., curve_fn=CURVE_IDENTITY, modulus=None,
                   matte_background=True):
  """Visualize a 1D image and a 1D weighting according to some colormap (vis.py:48-106).

  value [H,W] with a colormap, [H,W,3] with colormap None; weight [H,W] in [0, 1].  lo / hi: the bounds, the weighted
  percentiles 50 -+ percentile / 2 (widened by eps32) where None -- or 0: `lo or auto`, as the reference has it.  curve_fn
  is applied to value, lo and hi; with a modulus the value is wrapped instead of scaled."""
  value, weight = _f32(value), _f32(weight)
  curve = _curve_name(curve_fn)
  # Identify the values that bound the middle of `value' according to `weight`.
  lohi = weighted_percentile(value, weight, [50 - percentile / 2, 50 + percentile / 2])
  lohi = lohi + torch.tensor([-_F32_EPS, _F32_EPS], dtype=torch.float32, device=lohi.device)
  if lo:
    lohi[0] = float(lo)
  if hi:
    lohi[1] = float(hi)
  lut = None
  if colormap is not None:
    if value.dim() == 3 and value.shape[-1] != 1:
      raise ValueError(f'value must have 1 channel under a colormap but has {value.shape[-1]}')
    lut = colormap_lut(colormap, value.device)
  else:
    if value.dim() != 3:
      raise ValueError(f'value must have 3 dims but has {value.dim()}')
    if value.shape[-1] != 3:
      raise ValueError(f'value must have 3 channels but has {value.shape[-1]}')
  return ops.vis_cmap(value, lohi, curve=None if curve == 'identity' else curve, modulus=modulus, lut=lut,
                      acc=weight if matte_background else None)


def visualize_coord_mod(coords, acc):
  """Visualize the coordinate of each point within its "cell"."""
  return ops.vis_matte(None, _f32(acc), preop='coord_mod', origins=_f32(coords))


def _interp(x, xp, fp):
  """jnp.interp(x, xp, fp) along the last axis: x [n], xp [..., m], fp [..., m] -> [..., n]."""
  m = xp.shape[-1]
  xb = x.expand(xp.shape[:-1] + x.shape).contiguous()
  i = torch.clamp(torch.searchsorted(xp.contiguous(), xb, right=True), 1, m - 1)
  g = lambda a, k: torch.gather(a, -1, k)
  x0, x1, f0, f1 = g(xp, i - 1), g(xp, i), g(fp, i - 1), g(fp, i)
  dx, df = x1 - x0, f1 - f0
  flat = dx.abs() <= float(np.spacing(np.float32(_F32_EPS)))
  f = torch.where(flat, f0, f0 + (xb - x0) / torch.where(flat, torch.ones_like(dx), dx) * df)
  f = torch.where(xb < xp[..., :1], fp[..., :1], f)
  return torch.where(xb > xp[..., -1:], fp[..., -1:], f)


def _resample_avg(t, tp, vp):
  """stepfun.resample(t, tp, vp, use_avg=True) (stepfun.py:311-342): t [n+1], tp [R,m+1], vp [R,C,m] -> [R,C,n]."""
  wp = torch.diff(tp, dim=-1)[:, None, :]

  def summed(v):
    acc0 = torch.cat([torch.zeros_like(v[..., :1]), torch.cumsum(v, -1)], -1)
    return torch.diff(_interp(t, tp[:, None, :].expand(acc0.shape[:-1] + tp.shape[-1:]), acc0), dim=-1)

  return summed(vp * wp) / torch.clamp(summed(wp), min=_F32_EPS)


def visualize_rays(dist, dist_range, weights, rgbs, accumulate=False, renormalize=False, resolution=2048, bg_color=0.8):
  """Visualize a bundle of rays (vis.py:114-167): per level dist [R,m+1], weights [R,m], rgbs [R,m,C]; returns
  (vis [rows, cols, C], alpha [rows, cols]).  A few rays per image (Config.vis_num_rays): torch ops on the device."""
  dev = dist[0].device
  dist_vis = torch.linspace(float(dist_range[0]), float(dist_range[1]), resolution + 1, dtype=torch.float32, device=dev)
  vis_rgb, vis_alpha = [], []
  for ds, ws, rs in zip(dist, weights, rgbs):
    ds, ws, rs = _f32(ds), _f32(ws), _f32(rs)
    if accumulate:
      w_csum = torch.cumsum(ws, -1)
      rw_csum = torch.cumsum(rs * ws[..., None], -2)
      rs, ws = (rw_csum + _F32_EPS) / (w_csum[..., None] + 2 * _F32_EPS), w_csum
    vis_rgb.append(_resample_avg(dist_vis, ds, rs.transpose(-1, -2)).transpose(-1, -2))      # [R, resolution, C]
    vis_alpha.append(_resample_avg(dist_vis, ds, ws[:, None, :])[:, 0])                      # [R, resolution]
  vis_rgb = torch.stack(vis_rgb, 1)                              # [R, levels, resolution, C]
  vis_alpha = torch.stack(vis_alpha, 1)                          # [R, levels, resolution]
  if renormalize:
    # Scale the alphas so that the largest value is 1, for visualization.
    vis_alpha = vis_alpha / torch.clamp(vis_alpha.max(), min=_F32_EPS)
  n_rays, n_levels = vis_rgb.shape[:2]
  if resolution > n_rays:
    # every (ray, level) becomes `rep` image rows, and a strip of background rows follows each ray's levels
    rep = resolution // (n_rays * n_levels + 1)
    stride = rep * n_levels
    rgb_row, alpha_row = tuple(vis_rgb.shape[2:]), tuple(vis_alpha.shape[2:])
    vis_rgb = vis_rgb.repeat(1, 1, rep, 1).reshape((-1, stride) + rgb_row)
    vis_alpha = vis_alpha.repeat(1, 1, rep).reshape((-1, stride) + alpha_row)
    vis_rgb = torch.cat([vis_rgb, torch.zeros_like(vis_rgb[:, :1])], 1).reshape((-1,) + rgb_row)
    vis_alpha = torch.cat([vis_alpha, torch.zeros_like(vis_alpha[:, :1])], 1).reshape((-1,) + alpha_row)
  # Matte the RGB image over the background.
  vis = vis_rgb * vis_alpha[..., None] + (bg_color * (1 - vis_alpha))[..., None]
  # Remove the final row of background pixels.
  return vis[:-1], vis_alpha[:-1]


def visualize_suite(rendering, rays, cmaps=None):
  """A wrapper around other visualizations for easy integration (vis.py:170-260).  rendering: the dict of
  models.render_image; rays: the [H,W,.] rays it was rendered from.  cmaps: optional {name: [n,3] table} standing in for
  the matplotlib colormaps 'turbo' and 'gray'."""
  cmaps = cmaps or {}
  cmap = lambda name: cmaps.get(name, name)
  rgb = _f32(rendering['rgb'])
  distance_mean = _f32(rendering['distance_mean'])
  distance_median = _f32(rendering['distance_median'])
  distance_p5 = _f32(rendering['distance_percentile_5'])
  distance_p95 = _f32(rendering['distance_percentile_95'])
  acc = _f32(rendering['acc'])
  acc = torch.where(torch.isnan(distance_mean), torch.zeros_like(acc), acc)

  vis_depth_mean, vis_depth_median = [
      visualize_cmap(x, acc, cmap('turbo'), curve_fn=CURVE_NEG_LOG) for x in [distance_mean, distance_median]
  ]

  # Render three depth percentiles directly to RGB channels, where the spacing
  # determines the color. delta == big change, epsilon = small change.
  #   Gray: A strong discontinuitiy, [x-epsilon, x, x+epsilon]
  #   Purple: A thin but even density, [x-delta, x, x+delta]
  #   Red: A thin density, then a thick density, [x-delta, x, x+epsilon]
  #   Blue: A thick density, then a thin density, [x-epsilon, x, x+delta]
  vis_depth_triplet = visualize_cmap(
      torch.stack([2 * distance_median - distance_p5, distance_median, distance_p95], -1), acc, None, curve_fn=CURVE_LOG)

  dist = rendering['ray_sdist']
  dist_range = (0, 1)
  weights = rendering['ray_weights']
  rgbs = [torch.clamp(r, 0, 1) for r in rendering['ray_rgbs']]

  vis_ray_colors, _ = visualize_rays(dist, dist_range, weights, rgbs)

  sqrt_weights = [torch.sqrt(w) for w in weights]
  sqrt_ray_weights, ray_alpha = visualize_rays(
      dist,
      dist_range,
      [torch.ones_like(lw) for lw in sqrt_weights],
      [lw[..., None] for lw in sqrt_weights],
      bg_color=0,
  )
  sqrt_ray_weights = sqrt_ray_weights[..., 0].contiguous()

  null_color = torch.tensor([1., 0., 0.], dtype=torch.float32, device=rgb.device)
  vis_ray_weights = torch.where(
      ray_alpha[:, :, None] == 0,
      null_color[None, None],
      visualize_cmap(
          sqrt_ray_weights,
          torch.ones_like(sqrt_ray_weights),
          cmap('gray'),
          lo=0,
          hi=1,
          matte_background=False,
      ),
  )

  vis = {
      'color': rgb,
      'acc': acc,
      'color_matte': matte(rgb, acc),
      'depth_mean': vis_depth_mean,
      'depth_median': vis_depth_median,
      'depth_triplet': vis_depth_triplet,
      'coords_mod': ops.vis_matte(None, acc, preop='coord_mod', origins=_f32(rays.origins), directions=_f32(rays.directions),
                                  distance=distance_mean),
      'ray_colors': vis_ray_colors,
      'ray_weights': vis_ray_weights,
  }

  if rendering.get('rgb_cc') is not None:
    vis['color_corrected'] = rendering['rgb_cc']

  # Render every item named "normals*".
  for key, val in rendering.items():
    if key.startswith('normals') and val is not None:
      vis[key] = ops.vis_matte(_f32(val), acc, preop='half')

  if rendering.get('roughness') is not None:
    vis['roughness'] = ops.vis_matte(_f32(rendering['roughness']), acc, preop='tanh')

  return vis
