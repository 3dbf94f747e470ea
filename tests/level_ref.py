"""Plain-torch restatement of one level's rendering, training losses and sample-distance warp (TEST INFRASTRUCTURE ONLY).

What csrc/render.hip, csrc/ray_losses.h and csrc/losses.hip compute, written from the reference's definitions
(models.py:257-267, 462-464, 506, 584-602; render.py:130-213; train_utils.py:72-159; stepfun.py:64-86, 266-276;
coord.py:63-99) with whole-batch tensor ops and differentiated by autograd: no scan, no search, no hand-written VJP.
Every function takes `dtype`: float64 is the reference the leaf tests (tests/test_gpu_level_leaf.py) hold the kernels to,
float32 is the yardstick (the same statements, which are the oracle's own functions wherever the oracle has one, in the
kernels' number format; the rendering's sums along the ray are then taken term by term, see `cumsum_ray`).  Inputs are
rounded to fp32 first (`x.float().to(dtype)`), so both see the numbers the kernel sees.
"""

import torch

from oracle import coord as ocoord
from oracle import render as orender
from oracle import stepfun as ostepfun
from oracle import train_utils as otrain

ACTS = ('sigmoid', 'safe_exp', 'softplus', 'exp', 'relu', 'identity')                 # the keys of _lib.ACT
RAYDISTS = (None, 'identity', 'reciprocal', 'piecewise', 'log', 'exp', 'sqrt', 'square')   # the keys of _lib.RAYDIST


def cast(x, dtype):
  """A test input as the kernel sees it (fp32), in the arithmetic's dtype; a fresh leaf-able tensor."""
  return None if x is None else x.detach().float().to(dtype).clone()


def act(kind, x):
  if kind == 'sigmoid':
    return torch.sigmoid(x)
  if kind == 'safe_exp':                 # exp(min(x, 88)), whose derivative is its own value also where the clip acts
    return torch.exp(x + (torch.clamp(x, max=88.0) - x).detach())
  if kind == 'softplus':
    return torch.nn.functional.softplus(x)
  if kind == 'exp':
    return torch.exp(x)
  if kind == 'relu':
    return torch.relu(x)
  if kind == 'identity':
    return x
  raise ValueError(kind)


def cumsum_ray(x):
  """Cumulative sum over the last axis, differentiable.  In float32 term by term, each partial sum rounded to fp32, as numpy
  and the kernels do and as oracle.stepfun.seq_cumsum states it: torch's CPU cumsum accumulates fp32 rows in double and
  its sum adds in blocks, so their error does not grow with n and would not measure what an fp32 sum of n terms costs."""
  if x.dtype == torch.float64 or x.shape[-1] == 0:
    return torch.cumsum(x, dim=-1)
  out, run = [], torch.zeros_like(x[..., 0])
  for i in range(x.shape[-1]):
    run = run + x[..., i]
    out.append(run)
  return torch.stack(out, dim=-1)


def sum_ray(x):
  """Sum over the last axis, in the order and precision of `cumsum_ray`."""
  return torch.sum(x, dim=-1) if x.dtype == torch.float64 else cumsum_ray(x)[..., -1]


def forward(cfg, raw_density, tdist, dirs, *, raw_rgb=None, noise=None, bg=None, expo=None, dtype=torch.float64):
  """One level's rendering.  `cfg` holds the keyword arguments of ops.composite_cfg; the tensors are leaves already cast
  (see `cast`), so that the caller can ask autograd for their gradients.  Returns density, x (= density * delta, the optical
  depth increments BEFORE the opaque last sample is planted: a non-leaf kept for d / d x), rgb [B, n, 3] | None, weights,
  rgb_out, acc."""
  raw = raw_density
  if noise is not None and cfg['density_noise_std'] > 0:
    raw = raw + cfg['density_noise_std'] * noise                                       # models.py:462-464
  density = act(cfg['density_act'], raw + cfg['density_bias'])                         # models.py:506
  delta = (tdist[..., 1:] - tdist[..., :-1]) * torch.linalg.norm(dirs[..., None, :], dim=-1)
  x = density * delta
  if x.requires_grad:
    x.retain_grad()
  xs = x
  if cfg['opaque_background']:
    xs = torch.cat([x[..., :-1], torch.full_like(x[..., -1:], float('inf'))], dim=-1)
  alpha = 1 - torch.exp(-xs)
  trans = torch.exp(-torch.cat([torch.zeros_like(xs[..., :1]), cumsum_ray(xs[..., :-1])], dim=-1))
  weights = alpha * trans                                                              # render.py:130-151
  rgb = None
  if cfg['has_rgb']:
    rgb = act(cfg['rgb_act'], cfg['rgb_premultiplier'] * raw_rgb + cfg['rgb_bias'])    # models.py:584-586
    rgb = rgb * (1 + 2 * cfg['rgb_padding']) - cfg['rgb_padding']                      # models.py:602
    if expo is not None:
      rgb = rgb * expo[:, None, :]                                                     # models.py:257-267
  rgbs = rgb if rgb is not None else torch.zeros(weights.shape + (3,), dtype=dtype)
  bgv = bg if cfg['bg_mode'] == 1 else torch.full((weights.shape[0], 3), cfg['bg_value'], dtype=dtype)
  acc = sum_ray(weights)                                                               # render.py:154-181
  bg_w = torch.clamp(1 - acc[..., None], min=0)
  rgb_out = sum_ray((weights[..., None] * rgbs).transpose(-1, -2)) + bg_w * bgv
  return dict(density=density, x=x, rgb=rgb, weights=weights, rgb_out=rgb_out, acc=acc)


def exposure_scale(ev, idx, offsets, dtype=torch.float64):
  """models.py:257-267 folded into one [B, 3] factor: exposure_values * (1 + [idx > 0] * offsets[idx])."""
  ev = ev.to(dtype)
  sc = torch.ones((ev.shape[0], 3), dtype=dtype)
  if offsets is not None:
    on = (idx > 0)[:, None].to(dtype)
    sc = 1 + on * offsets.to(dtype)[idx.clamp(min=0).long()]
  return ev[:, None] * sc


def extras(weights, tdist, t_far):
  """render.py:184-211: distance_mean and the 5 / 50 / 95 percentiles, [B, 4], in the arguments' dtype."""
  B, n = weights.shape
  r = orender.volumetric_rendering(torch.zeros((B, n, 3), dtype=weights.dtype), weights, tdist, 0.0, t_far.reshape(B, 1), True)
  return torch.stack([r['distance_mean'], r['distance_percentile_5'], r['distance_median'], r['distance_percentile_95']], -1)


def lossmult_sum(lossmult, B_valid):
  """The data losses' denominator: the sum of lossmult over the valid rays and three channels."""
  return lossmult[:B_valid].expand(B_valid, 3).sum()


def data_loss(loss_type, charb_padding, mult, rgb_out, gt, lossmult, B_valid):
  """train_utils.py:72-111 on the valid rays: (mse stat, mult * data loss)."""

  class Cfg:
    disable_multiscale_loss = False
    data_coarse_loss_mult = 0.0
    compute_disp_metrics = False
    compute_normal_metrics = False

  Cfg.charb_padding, Cfg.data_loss_mult, Cfg.data_loss_type = charb_padding, mult, loss_type

  class Obj:
    pass

  batch, rays = Obj(), Obj()
  batch.rgb, rays.lossmult = gt[:B_valid], lossmult[:B_valid]
  loss, st = otrain.compute_data_loss(batch, [{'rgb': rgb_out[:B_valid]}], rays, Cfg)
  return st['mses'][0], loss


def interlevel_loss(mult, t_ref, w_ref, sdist, weights, B_valid):
  """train_utils.py:139-150: (sdist, weights) must envelope the final level's (t_ref, w_ref); mean over [B_valid, n_ref]."""
  return mult * torch.mean(ostepfun.lossfun_outer(t_ref[:B_valid], w_ref[:B_valid], sdist[:B_valid], weights[:B_valid]))


def distortion_loss(mult, sdist, weights, B_valid):
  """train_utils.py:153-159: mean over the valid rays."""
  return mult * torch.mean(ostepfun.lossfun_distortion(sdist[:B_valid], weights[:B_valid]))


def s_to_t(raydist_fn, sdist, near, far):
  """coord.py:96-98 for every entry of _lib.RAYDIST; near / far are [B]."""
  fn = None if raydist_fn in (None, 'identity') else raydist_fn
  return ocoord.construct_ray_warps(fn, near[:, None], far[:, None])[1](sdist)
