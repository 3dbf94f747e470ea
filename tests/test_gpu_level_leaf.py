"""Leaf tests of the per-ray level kernels against fp64, one gradient term at a time.  -m gpu.

composite_fwd_kernel<LPR>, level_bwd_kernel<LPR>, sdist_bwd_kernel, render_extras_kernel and the exposure kernel
(csrc/render.hip), the shared loss pieces (csrc/ray_losses.h), the stand-alone loss kernels (csrc/losses.hip) and
mnr_weighted_sum, each against tests/level_ref.py in float64 (plain torch + autograd, inputs rounded to fp32 first).

The figure of an output tensor is, per ray, max |got - ref64| / max |ref64| over the ray's entries, and the worst ray
counts (a ray whose fp64 values are all zero is measured at the largest ray's scale: the stand-alone interlevel kernel adds
and then subtracts the gradient factors of histogram bins that lie outside the envelope, which leaves their rounding
behind; a tensor that is all zero in fp64 must come out exactly zero).  The YARDSTICK is the same figure of the fp32
oracle (tests/level_ref.py in float32: oracle/ in the kernels' own number format, with the rendering's sums along the ray
taken term by term as the kernels and numpy take them, because torch's CPU cumsum accumulates fp32 in double) on the same
inputs against the same fp64 values.  A kernel passes when

    figure <= MARGIN * yardstick,    MARGIN = 8

The margin covers blocked instead of sequential sums and the device's expf / logf (1-2 ulp) against the host's.  A floor
stands beside 8 x the yardstick ONLY where the oracle's own chain is a few roundings long, so that its error comes out as a
fraction of an ulp, or 0, by luck (every output that passes by a floor, its error above 8 x the yardstick, is printed with a ^):
  * n <= 2, every output: 16 x 2^-24 forward (raw + bias, the activation's exp and log1p at up to 2 ulp each on the device,
    |d| (3 products, 2 sums, sqrt), the interval, delta, x, the two exponentials, 1 - ., the product: 18 roundings of half an
    ulp, most of them damped), 32 x 2^-24 backward (the VJP recomputes that chain and adds g^, T_{i+1}, two products, the
    difference, delta x act');
  * the scalar loss values (mse, data loss, lossmult_sum, interlevel and distortion loss), 2 (16 + sqrt n) x 2^-24: torch sums
    them in blocks and rounds the scalar about once (yardsticks of 5e-10 to 7e-8: about half an ulp), while the kernels'
    value is the backward chain above (32) and then a term-by-term fp32 sum per lane (for the distortion loss of n x n
    products, n of them in the inner sum: independent roundings add as a random walk, sqrt n each way), a 6-step wave sum,
    one atomic add per workgroup, the division and the multiplier.  These are the only outputs past 8 x the yardstick: at 1
    to 3 ulp on the simulator; on the MI355X the distortion loss value reads 1.2e-6 at n = 128 and 2.6e-6 at n = 288
    against yardsticks of 7e-8 and 6e-8.  They are logged statistics; no gradient is formed from them;
  * exposure_scale (two roundings): 4 x 2^-24; weighted_sum at n = 1: 2 x 2^-24.
No yardstick may exceed YARD_MAX = 2e-4 (asserted): above that a case measures the conditioning of its inputs, not a
kernel.  The largest are the interlevel gradients (1e-5 to 1.1e-4): the outer measure is a DIFFERENCE of two cumulative sums
of envelope weights (each rounded at ~3e-8 of their total), and the gradient factor 2 max(0, w - w_outer) / w inherits that
absolute error over a w - w_outer of ~1e-3; the kernels take the same difference.  A 5 % error there still fails every
interlevel case on both forms.  Three kinds of rays are ill-conditioned by construction and are handled by themselves:
  * the planted empty ray without the opaque last sample (forward): its weights are ~1e-13 in fp64 and exactly 0 in fp32
    (1 - exp(-x) rounds at the scale of 1).  It is left out of the relative figure of `weights` and `acc` and held at that
    absolute scale (2^-24 per weight) and to the fp32 oracle exactly;
  * rawnerf on dark or negative colours: the loss has a pole at rgb_out = -1e-3 and d loss / d rgb_out of ~1e6 near 0, whose
    density gradient is the remainder of a cancelling sum; the rawnerf cases render positive colours (no padding, no identity
    or ReLU colours);
  * saturated rays in the backward cases (see below).
Every test prints `worst error / bound` per output and asserts that no ratio exceeds 1.  Values are compared exactly
(torch.equal) where the definition makes them exact: zeros of padded rays, the bf16 copy of the density gradient, a zero
loss, a gradient passed through unchanged.

Only ONE gradient source is active in a case (g_rgb_out, g_weights, one data loss, the interlevel loss, the distortion
loss), so each term is held at its own scale; one combined case checks the wiring.  Both kernel forms (four lanes per ray
and lane per ray, mnr_level_bwd_set_quad) run wherever the launcher allows the quad form.

Worst error / bound over the cases of each test, measured on the MI355X (all cases pass there and on the kernel-source
simulator):

  test (source)                         outputs
  fwd                                   density 0.14  rgb 0.17  weights 0.21  rgb_out 0.20  acc 0.29
  bwd_upstream, g_rgb_out               g_raw_density 0.55  g_raw_rgb 0.28  g_x 0.33  g_exposure_scale 0.34
  bwd_upstream, g_weights               g_raw_density 0.20  g_x 0.14  (colour and exposure gradients exactly 0)
  bwd_data_loss                         g_raw_density 0.57  g_raw_rgb 0.18  g_x 0.32  g_exposure_scale 0.80
                                        mse 0.09^  data loss 0.08^  lossmult_sum 0.04^
  bwd_distortion, fused                 g_raw_density 0.82  g_x 0.42  loss 0.89 (by the floor: 0.67^ at n = 288)
  bwd_distortion, stand-alone           g_w 0.33  loss 0.67^;  pushed through the VJP, under the fused bound: at most 0.63
  bwd_interlevel, fused                 g_raw_density 0.88  g_x 0.36  loss 0.14^
  bwd_interlevel, stand-alone           g_w 0.21  loss 0.14^
  bwd_combined_wiring                   g_raw_density 0.19  g_raw_rgb 0.10  g_x 0.11  g_exposure_scale 0.12  losses 0.05
  sdist_bwd                             g_x 0.22  (g_t0, g_t1) 0.20  distortion 0.40
  render_extras                         mean 0.27  5% 0.12  median 0.26  95% 0.52
  weighted_sum 0.35   exposure_scale 0.12
  standalone_losses_128                 interlevel loss 0.03  distortion loss 0.01  g_w_env 0.06  g_w 0.30
                                        lossfun_outer 0.14  lossfun_distortion 0.27

^ Outputs that pass by a floor, i.e. whose error is above 8 x the yardstick, on the MI355X: loss VALUES only, in 20 of the
~950 output checks: mse (7 data-loss cases at n <= 128, 1 to 3 ulp), data loss (2), lossmult_sum (1), the distortion loss
value (fused and stand-alone at n = 3, 5, 31, 128, 288: up to 2.6e-6 at n = 288 against a yardstick of 6e-8), the
interlevel loss value at n = 7, n_ref = 3 (2 ulp).  Every tensor output, forward and gradient, at every n > 2 is inside
8 x the yardstick.

Two things about the cases themselves:
  * The data loss is a function of rgb_out, which is an INPUT of mnr_level_bwd (the forward kernel's output).  The reference
    takes the loss and d loss / d rgb_out at that fp32 number, as it takes every other input, and pushes the gradient through
    its own fp64 rendering.  Taken at the reference's own fp64 rgb_out instead, the residual y - gt carries the forward pass's
    rounding amplified by |y| / |y - gt| (9e-6 at n = 288 with charb, against a yardstick of 3e-7): the conditioning of the
    subtraction, which no backward kernel can be held to.
  * The backward inputs keep every ray away from saturation (|1 - acc| > 1e-4 without the opaque last sample, asserted):
    the background term's gate [acc < 1] is decided on the fp32 sum of the weights, and on a ray whose fp64 acc is within
    rounding of 1 all gradients are ~1e-12 of the batch's and the gate's tie decides them whole.  The saturated, the empty
    and the acc >= 1 rays are planted in the forward cases, where they have values to hold.
"""

import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import level_ref as R

U = 2.0 ** -24
MARGIN = 8.0


YARD_MAX = 2e-4          # a yardstick above this measures the conditioning of the inputs, not a kernel: such inputs are a mistake


def floor_scalar(n):
  """Loss values: see the module docstring."""
  return 2 * (16 + math.sqrt(n)) * U


def floor_fwd(n):
  """Only where the oracle's own chain is a few roundings long (n <= 2); else None: 8 x the yardstick alone."""
  return 16 * U if n <= 2 else None


def floor_bwd(n):
  return 32 * U if n <= 2 else None


f64, f32 = torch.float64, torch.float32


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from multinerf_amd import ops as _ops
  _ops.lib()
  return _ops


@pytest.fixture(autouse=True)
def _default_form_afterwards(ops):
  yield
  ops.L.check(ops.L.debug().mnr_level_bwd_set_quad(1))


def _set_form(ops, form):
  """'quad': four lanes per ray where 16 rays fit the launcher's LDS limit (else the launcher itself takes one lane per ray);
  'lane': one lane per ray for every shape."""
  ops.L.check(ops.L.debug().mnr_level_bwd_set_quad(1 if form == 'quad' else 0))


def dev(x):
  return None if x is None else x.contiguous().cuda()


# ----------------------------------------------------------------------------- figures and bounds


def _figure(got, ref, skip=()):
  """Worst ray's max |got - ref| / max |ref|; `skip`: rays held some other way by the caller."""
  ref = ref.detach().double().cpu()
  got = got.detach().double().cpu()
  assert got.numel() == ref.numel(), (got.shape, ref.shape)
  rows = ref.shape[0] if ref.dim() >= 1 and ref.numel() > 0 else 1
  ref, got = ref.reshape(rows, -1), got.reshape(rows, -1)
  if skip:
    keep = [r for r in range(rows) if r not in skip]
    ref, got = ref[keep], got[keep]
  assert torch.isfinite(ref).all(), 'the fp64 reference must be finite'
  scale = ref.abs().amax(1)
  scale = torch.where(scale > 0, scale, scale.max())     # a ray that is all zero in fp64 has no scale of its own: the batch's
  err = torch.nan_to_num((got - ref).abs(), nan=math.inf).amax(1)
  fig = torch.where(scale > 0, err / scale.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
  return fig.max().item()


def _ratio(fig, bound):
  return fig / bound if bound > 0 else (0.0 if fig == 0 else math.inf)     # (a bound of 0: exact zeros on both sides)


def _hold(label, items):
  """items: (name, got, ref64, ref32, floor | None[, rays to skip]).  Prints worst error / bound per output (marked ^ where
  it passes by the floor: the error is above 8 x the yardstick), asserts every ratio <= 1; returns the bounds by name."""
  parts, bad, bounds = [], [], {}
  for name, got, r64, r32, floor, *rest in items:
    skip = rest[0] if rest else ()
    fig, yard = _figure(got, r64, skip), _figure(r32, r64, skip)
    assert yard <= YARD_MAX, f'{label} {name}: the fp32 oracle is off by {yard:.3e} here: ill-conditioned inputs'
    bound = max(MARGIN * yard, floor or 0.0)
    bounds[name] = bound
    ratio = _ratio(fig, bound)
    parts.append(f'{name} {ratio:.3f}' + ('^' if fig > MARGIN * yard else ''))
    if not ratio <= 1.0:
      bad.append(f'{name}: error {fig:.3e} > bound {bound:.3e} (fp32 oracle {yard:.3e})')
  print(f'{label}: worst error / bound ' + ' '.join(parts))
  assert not bad, f'{label}: ' + '; '.join(bad)
  return bounds


# ----------------------------------------------------------------------------- inputs

SMALL = [(1, 3), (2, 17), (3, 5), (5, 33), (31, 16), (33, 1)]     # (n, B): no n is a multiple of the four lanes of a ray
BIG = [(128, 18), (288, 37), (1024, 3)]   # 128 with colour: the quad block needs more than 64 KiB backward; 288: the launcher itself
                                          # takes one lane per ray; 1024: LDS cuts the rays of a workgroup to 4 forward, 2 backward


def _cfg(k, flip=0, has_rgb=True):
  """Row k of the configuration table: density / colour activation k and k + 1 of _lib.ACT; the switches (opaque last
  sample, noise, exposure, background by tensor, non-trivial premultiplier / bias / padding) on when k + flip is odd."""
  on = (k + flip) & 1
  cfg = dict(opaque_background=bool(on), density_act=R.ACTS[k % 6], density_bias=-1.0 if on else 0.5,
             density_noise_std=0.5 if on else 0.0, has_rgb=has_rgb, rgb_act=R.ACTS[(k + 1) % 6],
             rgb_premultiplier=0.7 if on else 1.0, rgb_bias=-0.3 if on else 0.0, rgb_padding=0.01 if on else 0.0,
             bg_mode=on, bg_value=0.0 if on else 0.25)
  return cfg, dict(noise=bool(on), expo=bool(on))


def _inputs(seed, n, B, cfg, use, plant):
  """Random rays with the edge rays planted (`plant`: 'fwd' all five, 'bwd' the zero-width interval and the zero direction
  only: behind a saturated sample the fp64 gradient is ~1e-50 of nothing, which no fp32 code can be held to per ray)."""
  g = torch.Generator().manual_seed(seed)
  raw_d = torch.randn((B, n), generator=g) * (2 if plant == 'fwd' else 1)
  raw_rgb = torch.randn((B, n, 3), generator=g)
  s = torch.cumsum(torch.rand((B, n + 1), generator=g, dtype=f64) + 1e-3, -1)
  sdist = ((s - s[:, :1]) / (s[:, -1:] - s[:, :1])).float()
  dirs = torch.randn((B, 3), generator=g)
  bg = torch.rand((B, 3), generator=g)
  expo = 0.5 + torch.rand((B, 3), generator=g)
  noise = torch.randn((B, n), generator=g)
  k = min(1, n - 1)
  sdist[0, k + 1] = sdist[0, k]                                        # a zero-width interval
  tdist = (0.2 + (5.8 if plant == 'fwd' else 1.0) * sdist).float()
  if plant != 'fwd':                                                   # backward: |d| in [0.5, 1.5], optical depths of a few units, so
    dirs = dirs / torch.linalg.norm(dirs, dim=-1, keepdim=True) * (0.5 + torch.rand((B, 1), generator=g))   # that no ray saturates
  if B > 1:
    dirs[1] = 0.0                                                      # a zero direction vector
  if plant == 'fwd':
    if B > 2:                                                          # a saturated sample: everything behind it at T = 0
      raw_d[2] = torch.randn(n, generator=g)
      raw_d[2, min(2, n - 1)] = 30.0
      noise[2] = 0.0
      tdist[2] = 0.2 + torch.arange(n + 1, dtype=f32)                  # unit intervals, |d| = 4
      dirs[2] = torch.tensor([0.0, 4.0, 0.0])
    if B > 3:                                                          # an empty ray (identity has no empty value but 0)
      raw_d[3] = -cfg['density_bias'] if cfg['density_act'] in ('identity',) else -30.0
      noise[3] = 0.0
    if B > 4:                                                          # acc rounds to >= 1 without the opaque last sample
      raw_d[4] = 30.0
      noise[4] = 0.0
      dirs[4] = torch.tensor([8.0, 0.0, 0.0])
  d = dict(n=n, B=B, raw_d=raw_d, raw_rgb=raw_rgb if cfg['has_rgb'] else None, sdist=sdist, tdist=tdist, dirs=dirs,
           bg=bg if cfg['bg_mode'] == 1 else None, expo=expo if (use['expo'] and cfg['has_rgb']) else None,
           noise=noise if use['noise'] else None)
  return d


def _ref_forward(cfg, inp, dtype, grad=False):
  c = lambda k: R.cast(inp[k], dtype)
  leaves = dict(raw_d=c('raw_d'), raw_rgb=c('raw_rgb'), expo=c('expo'))
  if grad:
    for v in leaves.values():
      if v is not None:
        v.requires_grad_(True)
  f = R.forward(cfg, leaves['raw_d'], c('tdist'), c('dirs'), raw_rgb=leaves['raw_rgb'], noise=c('noise'), bg=c('bg'),
                expo=leaves['expo'], dtype=dtype)
  if grad:
    f['weights'].retain_grad()
  return leaves, f


def _kernel_forward(ops, cfg, inp):
  c = ops.composite_cfg(inp['n'], **cfg)
  kw = dict(raw_rgb=dev(inp['raw_rgb']), density_noise=dev(inp['noise']), bg=dev(inp['bg']), exposure_scale=dev(inp['expo']))
  a = (dev(inp['raw_d']), dev(inp['tdist']), dev(inp['dirs']))
  den, rgb, w, rgb_out, acc = ops.composite_fwd(c, *a, **kw)
  return c, a, kw, dict(density=den, rgb=rgb, weights=w, rgb_out=rgb_out, acc=acc)


# ----------------------------------------------------------------------------- forward

FWD_ROWS = []
for _k in range(6):
  FWD_ROWS.append((SMALL[_k], 'quad', _k, 0))
  FWD_ROWS.append((SMALL[(_k + 3) % 6], 'lane', _k, 1))
FWD_ROWS += [((128, 18), 'quad', 2, 1), ((200, 5), 'quad', 0, 0),      # 200 with colour: a quad block above 64 KiB forward
             ((288, 37), 'quad', 0, 1), ((1024, 3), 'quad', 2, 0)]


def _row_id(r):
  (n, B), form, k, flip = r
  return f'n{n}-B{B}-{form}-{R.ACTS[k % 6]}-{"on" if (k + flip) & 1 else "off"}'


def test_level_leaf_fwd_table_covers_every_value():
  """Each activation for density and for colour, and each switch in both positions, at an n that is no multiple of 4, on
  each kernel form."""
  for form in ('quad', 'lane'):
    rows = [(_cfg(k, flip), n) for (n, B), f, k, flip in FWD_ROWS if f == form and n % 4 != 0]
    for key in ('density_act', 'rgb_act'):
      assert {c[key] for (c, u), n in rows} == set(R.ACTS)
    for key in ('opaque_background', 'bg_mode'):
      assert {int(c[key]) for (c, u), n in rows} == {0, 1}
    assert {u['noise'] for (c, u), n in rows} == {True, False} and {u['expo'] for (c, u), n in rows} == {True, False}
    assert {c['rgb_padding'] > 0 for (c, u), n in rows} == {True, False}


@pytest.mark.parametrize('row', FWD_ROWS, ids=_row_id)
def test_level_leaf_fwd(ops, row):
  (n, B), form, k, flip = row
  cfg, use = _cfg(k, flip)
  inp = _inputs(100 + k, n, B, cfg, use, 'fwd')
  _, r64 = _ref_forward(cfg, inp, f64)
  _, r32 = _ref_forward(cfg, inp, f32)
  _set_form(ops, form)
  _, _, _, got = _kernel_forward(ops, cfg, inp)
  torch.cuda.synchronize()
  names = ['density', 'rgb', 'weights', 'rgb_out', 'acc'] if cfg['has_rgb'] else ['density', 'weights', 'rgb_out', 'acc']
  # The planted empty ray without the opaque last sample has weights of ~1e-13 in fp64 and exactly 0 in fp32 (1 - exp(-x)
  # rounds at the scale of 1), so it has no relative figure: it is held at that absolute scale, and to the fp32 oracle exactly.
  empty = (3,) if B > 3 and not cfg['opaque_background'] else ()
  _hold(f'level_leaf_fwd {_row_id(row)}', [(nm, got[nm], r64[nm], r32[nm], floor_fwd(n), empty if nm in ('weights', 'acc') else ())
                                           for nm in names])
  for r in empty:
    assert (got['weights'][r].cpu().double() - r64['weights'][r]).abs().max().item() <= U
    assert torch.equal(got['weights'][r].cpu(), r32['weights'][r]) and abs(got['acc'][r].item() - r64['acc'][r].item()) <= n * U
  if B > 4 and not cfg['opaque_background'] and cfg['density_act'] not in ('sigmoid',):
    assert got['acc'][4].item() >= 1.0 and r64['acc'][4].item() <= 1.0         # the planted ray does what it is planted for
  if B > 3 and not cfg['opaque_background']:
    assert got['acc'][3].item() < 1e-6


# ----------------------------------------------------------------------------- backward, one source at a time

DATA_VARIANTS = [('mse', 1), ('rawnerf', 3), ('charb', 3), ('rawnerf', 1), ('charb', 1), ('mse', 3)]


def _sources(inp, Bv, seed):
  g = torch.Generator().manual_seed(seed)
  B, n = inp['B'], inp['n']
  return dict(G=torch.randn((B, 3), generator=g), GW=torch.randn((B, n), generator=g), gt=torch.rand((B, 3), generator=g),
              lm1=torch.rand((B, 1), generator=g) + 0.1, lm3=torch.rand((B, 3), generator=g) + 0.1)


def _objective(spec, f, src, inp, Bv, dtype, extra):
  """The one term named by `spec` (or all of them for 'combined') of the reference objective, and its loss values."""
  kind = spec[0]
  c = lambda x: R.cast(x, dtype)
  obj, stats = 0.0, {}
  if kind in ('g_rgb_out', 'combined'):
    obj = obj + (f['rgb_out'] * c(src['G'])).sum()
  if kind in ('g_weights', 'combined'):
    obj = obj + (f['weights'] * c(src['GW'])).sum()
  if kind in ('data', 'combined'):
    lm = c(src['lm1'] if spec[2] == 1 else src['lm3'])
    # rgb_out is an INPUT of mnr_level_bwd (the forward kernel's output): the loss and d loss / d rgb_out are taken at that
    # number, as every other input is, and pushed through the reference's own rendering.  (At the reference's own rgb_out the
    # residual y - gt would carry the forward pass's rounding amplified by |y| / |y - gt|.)
    y = c(extra['y']).requires_grad_(True)
    mse, dl = R.data_loss(spec[1], 0.001, 0.7, y, c(src['gt']), lm, Bv)
    stats['mse'], stats['data_loss'] = mse, dl
    stats['denom'] = R.lossmult_sum(lm, Bv)
    obj = obj + (f['rgb_out'] * torch.autograd.grad(dl, y)[0]).sum()
  if kind in ('distortion', 'combined'):
    wl = R.distortion_loss(0.01, c(inp['sdist']), f['weights'], Bv)
    stats['wloss'] = wl
    obj = obj + wl
  if kind == 'interlevel':
    wl = R.interlevel_loss(1.0, c(extra['t_ref']), c(extra['w_ref']), c(inp['sdist']), f['weights'], Bv)
    stats['wloss'] = wl
    obj = obj + wl
  return obj, stats


def _ref_backward(cfg, inp, spec, src, Bv, dtype, extra=None):
  leaves, f = _ref_forward(cfg, inp, dtype, grad=True)
  obj, stats = _objective(spec, f, src, inp, Bv, dtype, extra)
  obj.backward()
  if not cfg['opaque_background']:                       # the background gate [acc < 1] is nowhere near its tie
    assert ((1 - f['acc'].detach()).abs() > 1e-4).all(), 'a ray of the backward inputs saturates'
  z = lambda t, like: torch.zeros_like(like) if t is None else t
  out = dict(g_rd=z(leaves['raw_d'].grad, leaves['raw_d']), g_x=z(f['x'].grad, f['x']), g_w=z(f['weights'].grad, f['weights']))
  if leaves['raw_rgb'] is not None:
    out['g_rr'] = z(leaves['raw_rgb'].grad, leaves['raw_rgb'])
  if leaves['expo'] is not None:
    out['g_ex'] = z(leaves['expo'].grad, leaves['expo'])
  out.update({k: v.detach() for k, v in stats.items()})
  out['fwd'] = f
  return out


def _kernel_backward(ops, cfg, inp, spec, src, Bv, extra=None, g_weights=None):
  """composite_fwd, then ONE mnr_level_bwd launch with the sources of `spec`; every output it has."""
  c, a, kw, fwd = _kernel_forward(ops, cfg, inp)
  B, n = inp['B'], inp['n']
  kind = spec[0]
  gbf = torch.zeros((B * n, 8), dtype=torch.bfloat16).cuda()
  g_ex = torch.zeros((B, 3)).cuda() if inp['expo'] is not None else None
  g_x = torch.full((B, n), math.nan).cuda()
  stats = torch.zeros(3).cuda()
  denom = torch.zeros(1).cuda()
  losses = None
  if kind in ('data', 'combined', 'distortion', 'interlevel'):
    losses = dict(B_valid=Bv, data=None, weights=None)
  if kind in ('data', 'combined'):
    lm = dev(src['lm1'] if spec[2] == 1 else src['lm3'])
    ops.lossmult_sum(lm, Bv, denom)
    losses['data'] = dict(type=spec[1], charb_padding=0.001, mult=0.7, rgb_out=fwd['rgb_out'], gt=dev(src['gt']), lossmult=lm,
                          denom=denom, stats=stats[0:2])
  if kind in ('distortion', 'combined'):
    losses['weights'] = dict(mode='distortion', mult=0.01, sdist=dev(inp['sdist']), stat=stats[2:3])
  if kind == 'interlevel':
    losses['weights'] = dict(mode='interlevel', mult=1.0, sdist=dev(inp['sdist']), t_ref=dev(extra['t_ref']),
                             w_ref=dev(extra['w_ref']), stat=stats[2:3])
  gw = g_weights if g_weights is not None else (dev(src['GW']) if kind in ('g_weights', 'combined') else None)
  g_rd, g_rr = ops.composite_bwd(c, *a, fwd['weights'], g_rgb_out=dev(src['G']) if kind in ('g_rgb_out', 'combined') else None,
                                 g_weights=gw, g_den_bf16=gbf.view(-1)[3:], ld_bf16=8, g_exposure_scale=g_ex, losses=losses,
                                 g_x_out=g_x, **kw)
  torch.cuda.synchronize()
  bf = gbf.cpu()
  assert torch.equal(bf[:, 3].reshape(B, n), g_rd.cpu().to(torch.bfloat16)), 'the bf16 copy is not the rounded fp32 gradient'
  bf[:, 3] = 0
  assert not bf.any(), 'the bf16 copy wrote outside its column'
  out = dict(g_rd=g_rd, g_x=g_x, g_rr=g_rr, g_ex=g_ex, mse=stats[0], data_loss=stats[1], wloss=stats[2], denom=denom[0], fwd=fwd)
  return out


SCALARS = ('mse', 'data_loss', 'denom', 'wloss')


def _hold_backward(label, got, r64, r32, names):
  fl = floor_bwd(got['g_rd'].shape[1])
  return _hold(label, [(nm, got[nm], r64[nm], r32[nm], floor_scalar(got['g_rd'].shape[1]) if nm in SCALARS else fl)
                       for nm in names if nm in r64 and got.get(nm) is not None])


GRAD_NAMES = ['g_rd', 'g_rr', 'g_x', 'g_ex']
BWD_SHAPES = [(s, f) for s in SMALL + BIG[:1] for f in ('quad', 'lane')] + [(s, 'quad') for s in BIG[1:]]


def _bwd_cfg(case, shift=0):
  """Shape si on form fi takes row si + 3 fi of the configuration table: all six activations, for density and for colour,
  and both positions of every switch on either form."""
  (n, B), form = case
  si, fi = (SMALL + BIG).index((n, B)), int(form == 'lane')
  return _cfg(si + 3 * fi + shift, fi)


def test_level_leaf_bwd_table_covers_every_value():
  """Each activation for density and, with colour present, for colour, and each switch in both positions, on each kernel
  form, at an n that is no multiple of 4 (levels without colour: n = 31 in test_level_leaf_bwd_upstream, the interlevel cases)."""
  for form in ('quad', 'lane'):
    rows = [_bwd_cfg(c) for c in BWD_SHAPES if c[1] == form and c[0][0] % 4 != 0]
    assert {c['density_act'] for c, u in rows} == set(R.ACTS)
    assert {c['rgb_act'] for c, u in rows if c['has_rgb']} == set(R.ACTS)
    for key in ('opaque_background', 'bg_mode'):
      assert {int(c[key]) for c, u in rows} == {0, 1}
    assert {u['noise'] for c, u in rows} == {True, False} and {u['expo'] for c, u in rows if c['has_rgb']} == {True, False}


def _b_valids(B):
  return [B, 1, B - 1] if B in (17, 33) else [B]


def _shape_id(p):
  (n, B), form = p
  return f'n{n}-B{B}-{form}'


@pytest.mark.parametrize('case', list(enumerate(BWD_SHAPES)), ids=lambda c: _shape_id(c[1]))
def test_level_leaf_bwd_upstream(ops, case):
  """g_rgb_out alone, then g_weights alone: the compositing VJP, d / d exposure_scale and g_x.  At n = 31 also as a level
  without colour (a proposal level: g_rgb_out then acts through the background weight alone)."""
  i, ((n, B), form) = case
  _set_form(ops, form)
  for has_rgb in ((True, False) if n == 31 else (True,)):
    cfg, use = _bwd_cfg(case[1])
    cfg['has_rgb'] = has_rgb
    inp = _inputs(200 + i, n, B, cfg, use, 'bwd')
    src = _sources(inp, B, 300 + i)
    for kind in ('g_rgb_out', 'g_weights'):
      r64, r32 = (_ref_backward(cfg, inp, (kind,), src, B, dt) for dt in (f64, f32))
      got = _kernel_backward(ops, cfg, inp, (kind,), src, B)
      _hold_backward(f'level_leaf_bwd {kind} {_shape_id(case[1])} {cfg["density_act"]}/{cfg["rgb_act"] if has_rgb else "no colour"}',
                     got, r64, r32, GRAD_NAMES)


@pytest.mark.parametrize('case', list(enumerate(BWD_SHAPES)), ids=lambda c: _shape_id(c[1]))
def test_level_leaf_bwd_data_loss(ops, case):
  """One data loss alone (two of the six (type, lossmult channels) variants per shape, all six on either form), with an
  exposure scale of 2 on half the rays so that rendered colours lie on both sides of the rawnerf clip."""
  i, ((n, B), form) = case
  _set_form(ops, form)
  for v in (DATA_VARIANTS[i % 6], DATA_VARIANTS[(i + 3) % 6]):
    cfg, use = _bwd_cfg(case[1])
    if v[0] == 'rawnerf':
      # The rawnerf loss weighs by 1 / (1e-3 + y)^2: a pole at y = -1e-3, and at a dark pixel a d loss / d rgb_out of ~1e6
      # whose density gradient is what is left of a cancelling sum (with the opaque last sample sum_k w_k is constant).  It is
      # a loss on positive colours: no padding below 0, no identity or ReLU colours (the upstream cases and this shape's
      # other variant run those activations).
      cfg.update(rgb_padding=0.0, rgb_act='sigmoid' if cfg['rgb_act'] in ('identity', 'relu') else cfg['rgb_act'])
    inp = _inputs(400 + i, n, B, cfg, dict(use, expo=True), 'bwd')
    if inp['expo'] is not None:
      inp['expo'][::2] = 2.0
    src = _sources(inp, B, 500 + i)
    for Bv in _b_valids(B):
      spec = ('data',) + v
      got = _kernel_backward(ops, cfg, inp, spec, src, Bv)
      extra = dict(y=got['fwd']['rgb_out'].cpu())
      r64, r32 = (_ref_backward(cfg, inp, spec, src, Bv, dt, extra) for dt in (f64, f32))
      _hold_backward(f'level_leaf_bwd data {v[0]} lm_c={v[1]} {_shape_id(case[1])} B_valid={Bv}', got, r64, r32,
                     GRAD_NAMES + ['mse', 'data_loss', 'denom'])
      assert torch.equal(got['g_rd'][Bv:].cpu(), torch.zeros((B - Bv, n)))          # padded rays: no loss, no gradient
      if v[0] == 'rawnerf' and cfg['has_rgb'] and Bv >= 16:
        y = extra['y'][:Bv]
        assert (y > 1).any() and (y < 1).any() and (y > 0).all()                    # the clip gate is crossed


@pytest.mark.parametrize('case', list(enumerate(BWD_SHAPES)), ids=lambda c: _shape_id(c[1]))
def test_level_leaf_bwd_distortion(ops, case):
  """The distortion loss alone (n = 1: its intra-interval term alone), fused in mnr_level_bwd and stand-alone
  (mnr_distortion_loss on the kernel's weights, its gradient pushed through the VJP as g_weights)."""
  i, ((n, B), form) = case
  cfg, use = _bwd_cfg(case[1], 1)
  if n == 1:                                           # the intra-interval term alone needs a live sample: an opaque only sample has
    cfg.update(opaque_background=False, density_act='softplus')   # the constant weight 1, a ReLU below 0 no gradient at all
  inp = _inputs(600 + i, n, B, cfg, use, 'bwd')
  src = _sources(inp, B, 700 + i)
  _set_form(ops, form)
  for Bv in _b_valids(B):
    spec = ('distortion',)
    r64, r32 = (_ref_backward(cfg, inp, spec, src, Bv, dt) for dt in (f64, f32))
    got = _kernel_backward(ops, cfg, inp, spec, src, Bv)
    label = f'level_leaf_bwd distortion {_shape_id(case[1])} B_valid={Bv}'
    bounds = _hold_backward(label, got, r64, r32, GRAD_NAMES + ['wloss'])
    assert torch.equal(got['g_rd'][Bv:].cpu(), torch.zeros((B - Bv, n)))
    _standalone_agrees(ops, label, 'distortion', cfg, inp, src, Bv, got, r64, r32, bounds, None)


def _standalone_agrees(ops, label, mode, cfg, inp, src, Bv, got, r64, r32, bounds, extra):
  """The stand-alone loss kernel of csrc/losses.hip on the same input: its own d loss / d weights and loss value against fp64,
  and the fused kernel's results within the fused kernel's own bounds."""
  B, n = inp['B'], inp['n']
  w_k = got['fwd']['weights']
  st = torch.zeros(1).cuda()
  g_w = torch.zeros((B, n)).cuda()
  if mode == 'distortion':
    try:
      ops.distortion_loss(0.01, dev(inp['sdist']), w_k, st, g_w, B_valid=Bv)
    except ValueError as e:                            # the stand-alone kernel keeps 64 whole rays in LDS and says so itself
      assert 'n too large' in str(e) and n > 288, (n, str(e))
      print(f'{label}: no stand-alone comparison: {e}')
      return
  else:
    ops.interlevel_loss(1.0, dev(extra['t_ref']), dev(extra['w_ref']), dev(inp['sdist']), w_k, st, g_w, B_valid=Bv)
  torch.cuda.synchronize()
  _hold(label + ' stand-alone', [('g_w', g_w, r64['g_w'], r32['g_w'], floor_bwd(n)), ('wloss', st[0], r64['wloss'], r32['wloss'], floor_scalar(n))])
  assert torch.equal(g_w[Bv:].cpu(), torch.zeros((B - Bv, n)))
  # Both kernels within the SAME bounds of the same fp64 values: the stand-alone gradient pushed through the VJP is held to
  # the fused kernel's reference under the fused kernel's bound, and so is its loss value; the two then differ from each
  # other by at most twice that, which is printed.
  via = _kernel_backward(ops, cfg, inp, ('g_weights',), src, Bv, g_weights=g_w)
  for nm, a, b in (('g_rd', via['g_rd'], got['g_rd']), ('wloss', st[0], got['wloss'])):
    fig, mutual = _figure(a, r64[nm]), _figure(a, b)
    print(f'{label} stand-alone under the fused bound {nm}: {_ratio(fig, bounds[nm]):.3f}; against fused / twice the bound {_ratio(mutual, 2 * bounds[nm]):.3f}')
    assert fig <= bounds[nm], f'{label}: stand-alone {nm} misses the bound of the fused kernel: {fig:.3e} > {bounds[nm]:.3e}'
    assert mutual <= 2 * bounds[nm]


# ----------------------------------------------------------------------------- the interlevel loss

INTERLEVEL = [((1, 1), 17), ((3, 7), 33), ((7, 3), 5), ((5, 64), 17), ((64, 32), 33), ((128, 128), 18)]     # ((n, n_ref), B)


def _histogram(seed, n_ref, inp):
  """The final level's histogram (t_ref, w_ref) for the envelope (inp.sdist on [0, 1]): by ray on [-0.3, 1.4] (reaching below
  and above the envelope), [0.2, 0.7] (inside) or [0, 1]; an interior fence-post that IS a fence-post of sdist (the same
  fp32 number); a zero-width interval; exact zeros in w_ref."""
  g = torch.Generator().manual_seed(seed)
  B, n, sdist = inp['B'], inp['n'], inp['sdist']
  s = torch.cumsum(torch.rand((B, n_ref + 1), generator=g, dtype=f64) + 1e-3, -1)
  s = (s - s[:, :1]) / (s[:, -1:] - s[:, :1])
  lo = torch.tensor([-0.3, 0.2, 0.0], dtype=f64)[torch.arange(B) % 3][:, None]
  hi = torch.tensor([1.4, 0.7, 1.0], dtype=f64)[torch.arange(B) % 3][:, None]
  t = (lo + (hi - lo) * s).float()
  for r in range(B):
    if n >= 2 and n_ref >= 2 and r % 2 == 0:
      t[r, 1 + r % (n_ref - 1)] = sdist[r, 1 + r % (n - 1)]            # an interior tie of the searchsorted
  t = torch.sort(t, dim=-1).values
  if B > 3 and n_ref >= 2:
    t[3, n_ref // 2 + 1] = t[3, n_ref // 2]                            # a zero-width interval of the histogram
  w = (torch.softmax(torch.randn((B, n_ref), generator=g) * 2, -1) * 0.9).float()
  w[1::4, ::3] = 0.0                                                   # exact zeros
  return dict(t_ref=t, w_ref=w)


@pytest.mark.parametrize('form', ['quad', 'lane'])
@pytest.mark.parametrize('shape', INTERLEVEL, ids=lambda s: f'n{s[0][0]}-nref{s[0][1]}-B{s[1]}')
def test_level_leaf_bwd_interlevel(ops, shape, form):
  """The interlevel loss alone, fused (a binary search per fence-post) and stand-alone (cursors), each against fp64 and
  against each other."""
  (n, n_ref), B = shape
  i = INTERLEVEL.index(shape)
  cfg, use = _cfg(2, i % 2, has_rgb=(n == 128))                       # softplus; the opaque last sample, noise, ... off and on
  inp = _inputs(800 + i, n, B, cfg, use, 'bwd')
  extra = _histogram(900 + i, n_ref, inp)
  if n >= 2 and n_ref >= 2:
    assert (extra['t_ref'][:, 1:-1, None] == inp['sdist'][:, None, 1:-1]).any()
  src = _sources(inp, B, 1000 + i)
  _set_form(ops, form)
  for Bv in _b_valids(B):
    spec = ('interlevel',)
    r64, r32 = (_ref_backward(cfg, inp, spec, src, Bv, dt, extra) for dt in (f64, f32))
    got = _kernel_backward(ops, cfg, inp, spec, src, Bv, extra)
    label = f'level_leaf_bwd interlevel n={n} n_ref={n_ref} B={B} {form} B_valid={Bv}'
    bounds = _hold_backward(label, got, r64, r32, GRAD_NAMES + ['wloss'])
    assert torch.equal(got['g_rd'][Bv:].cpu(), torch.zeros((B - Bv, n)))
    _standalone_agrees(ops, label, 'interlevel', cfg, inp, src, Bv, got, r64, r32, bounds, extra)


@pytest.mark.parametrize('form', ['quad', 'lane'])
def test_level_leaf_interlevel_bounding_envelope_is_exactly_zero(ops, form):
  """An envelope that already bounds the histogram (w_ref = half the outer measure of the fp64 weights): the loss and every
  gradient are exactly 0, in fp64 and in both kernels."""
  from oracle import stepfun as ostepfun
  n, n_ref, B = 5, 7, 17
  cfg, use = _cfg(2, 1, has_rgb=False)
  inp = _inputs(1100, n, B, cfg, use, 'bwd')
  extra = _histogram(1101, n_ref, inp)
  _, f = _ref_forward(cfg, inp, f64)
  _, w_outer = ostepfun.inner_outer(R.cast(extra['t_ref'], f64), R.cast(inp['sdist'], f64), f['weights'])
  extra['w_ref'] = (0.5 * w_outer).float()
  src = _sources(inp, B, 1102)
  r64 = _ref_backward(cfg, inp, ('interlevel',), src, B, f64, extra)
  assert r64['wloss'].item() == 0.0 and not r64['g_rd'].any()
  _set_form(ops, form)
  got = _kernel_backward(ops, cfg, inp, ('interlevel',), src, B, extra)
  assert torch.equal(got['wloss'].cpu(), torch.zeros(()))
  assert torch.equal(got['g_rd'].cpu(), torch.zeros((B, n))) and torch.equal(got['g_x'].cpu(), torch.zeros((B, n)))
  st, g_w = torch.zeros(1).cuda(), torch.zeros((B, n)).cuda()
  ops.interlevel_loss(1.0, dev(extra['t_ref']), dev(extra['w_ref']), dev(inp['sdist']), got['fwd']['weights'], st, g_w, B_valid=B)
  assert torch.equal(st.cpu(), torch.zeros(1)) and torch.equal(g_w.cpu(), torch.zeros((B, n)))


@pytest.mark.parametrize('form', ['quad', 'lane'])
def test_level_leaf_bwd_combined_wiring(ops, form):
  """Every source at once (g_rgb_out, g_weights, a data loss, the distortion loss), B_valid < B: the terms add up."""
  n, B, Bv = 5, 33, 32
  cfg, use = _cfg(1, 0)
  inp = _inputs(1200, n, B, cfg, use, 'bwd')
  src = _sources(inp, B, 1201)
  spec = ('combined', 'charb', 3)
  _set_form(ops, form)
  got = _kernel_backward(ops, cfg, inp, spec, src, Bv)
  extra = dict(y=got['fwd']['rgb_out'].cpu())
  r64, r32 = (_ref_backward(cfg, inp, spec, src, Bv, dt, extra) for dt in (f64, f32))
  _hold_backward(f'level_leaf_bwd combined {form}', got, r64, r32, GRAD_NAMES + ['mse', 'data_loss', 'wloss'])


# ----------------------------------------------------------------------------- sdist_bwd

NEAR_FAR = {None: (0.2, 3.0), 'identity': (0.2, 3.0), 'reciprocal': (0.2, 3.0), 'piecewise': (0.3, 4.0), 'log': (0.2, 3.0),
            'exp': (0.2, 2.0), 'sqrt': (0.2, 3.0), 'square': (0.2, 3.0)}                 # piecewise: near < 1 < far, both branches


@pytest.mark.parametrize('shape', [(1, 70), (5, 17), (33, 3)], ids=lambda s: f'n{s[0]}-B{s[1]}')
@pytest.mark.parametrize('fn', R.RAYDISTS, ids=lambda f: str(f))
def test_level_leaf_sdist_bwd(ops, fn, shape):
  """d loss / d sdist from each source alone: g_x, (g_t0, g_t1), the distortion term (B_valid < B), g_sdist_in."""
  n, B = shape
  fi = R.RAYDISTS.index(fn)
  g = torch.Generator().manual_seed(1300 + 10 * fi + n)
  s = torch.cumsum(torch.rand((B, n + 1), generator=g, dtype=f64) + 1e-3, -1)
  sdist = ((s - s[:, :1]) / (s[:, -1:] - s[:, :1])).float()
  if n >= 2:
    sdist[0, 2] = sdist[0, 1] = sdist[0, 0]              # two zero-width intervals with EQUAL midpoints: the sign term is 0
  lo, hi = NEAR_FAR[fn]
  near = (lo + 0.2 * torch.rand(B, generator=g)).float()
  far = (hi + torch.rand(B, generator=g)).float()
  raw_d = torch.randn((B, n), generator=g) * 2
  noise = torch.randn((B, n), generator=g)
  dirs = torch.randn((B, 3), generator=g)
  w = (torch.softmax(torch.randn((B, n), generator=g) * 2, -1) * 0.9).float()
  GX, GT0, GT1, GS = (torch.randn(sh, generator=g) for sh in ((B, n), (B, n), (B, n), (B, n + 1)))
  act, bias, std = R.ACTS[fi % 6], -0.5, 0.5
  Bv = max(1, B - 1)

  def ref(kind, dtype):
    c = lambda x: R.cast(x, dtype)
    sd = c(sdist).requires_grad_(True)
    t = R.s_to_t(fn, sd, c(near), c(far))
    if kind == 'g_x':
      sigma = R.act(act, c(raw_d) + std * c(noise) + bias)
      x = sigma * (t[:, 1:] - t[:, :-1]) * torch.linalg.norm(c(dirs)[:, None, :], dim=-1)
      obj = (x * c(GX)).sum()
    elif kind == 'g_t':
      obj = (t[:, :-1] * c(GT0)).sum() + (t[:, 1:] * c(GT1)).sum()
    else:
      obj = R.distortion_loss(0.01, sd, c(w), Bv)
    obj.backward()
    return sd.grad

  def kernel(kind):
    kw = {}
    if kind == 'g_x':
      kw = dict(g_x=dev(GX), raw_density=dev(raw_d), density_noise=dev(noise), density_noise_std=std, density_bias=bias,
                density_act=act, dirs=dev(dirs))
    elif kind == 'g_t':
      kw = dict(g_t0=dev(GT0), g_t1=dev(GT1))
    elif kind == 'distortion':
      kw = dict(distortion_mult=0.01, weights=dev(w), B_valid=Bv)
    else:
      kw = dict(g_sdist_in=dev(GS))
    out = ops.sdist_bwd(dev(sdist), dev(near), dev(far), fn, **kw)
    torch.cuda.synchronize()
    return out

  items = [(kind, kernel(kind), ref(kind, f64), ref(kind, f32), floor_bwd(n)) for kind in ('g_x', 'g_t', 'distortion')]
  _hold(f'level_leaf_sdist_bwd {fn} n={n} B={B}', items)
  assert torch.equal(kernel('g_sdist_in').cpu(), GS)                    # passed through unchanged
  if B > Bv:
    assert torch.equal(items[2][1][Bv:].cpu(), torch.zeros((B - Bv, n + 1)))


# ----------------------------------------------------------------------------- render_extras, weighted_sum, exposure_scale


@pytest.mark.parametrize('n', [1, 2, 5, 32])
@pytest.mark.parametrize('B', [1, 65])
def test_level_leaf_render_extras(ops, n, B):
  """distance_mean and the three percentiles; planted rays use dyadic weights, so that their cumulative sums are exact in
  fp32 and fp64 alike and a percentile that meets a flat CDF does so in both."""
  g = torch.Generator().manual_seed(1400 + n)
  w = (torch.softmax(torch.randn((B, n + 1), generator=g) * 2, -1)[:, :n] * torch.rand((B, 1), generator=g)).float()
  t = (0.2 + torch.cumsum(torch.rand((B, n + 1), generator=g) * 0.3 + 1e-3, -1)).float()
  if B > 8:
    w[0] = 0.0
    t[0, 0] = t[0, 1] = 0.0                          # an empty ray whose first midpoint is 0: 0 * log 0 = NaN -> inf -> clamped
    w[1] = 0.6 if n >= 2 else 1.2                    # weights that sum past 1 inside the bin of the 95th percentile: the CDF clamp
    w[2] = 0.25 / n                                  # acc = 0.25 < 0.5: the median lies in the background bin
    w[3] = 0.75 / n if n & (n - 1) == 0 else 0.8 / n  # acc < 0.95: the 95th percentile lies in the background bin
    w[4] = 0.0
    w[4, 0] = 0.5
    w[4, -1] += 0.25                                 # a run of zero weights: flat CDF at 0.5 (n >= 3), right-most duplicate
    t[5, min(1, n - 1) + 1] = t[5, min(1, n - 1)]    # a zero-width interval
  far = (t[:, -1] + 10 * torch.rand(B, generator=g)).float()
  r64, r32 = (R.extras(R.cast(w, dt), R.cast(t, dt), R.cast(far, dt)) for dt in (f64, f32))
  out = ops.render_extras(dev(w), dev(t), dev(far))
  torch.cuda.synchronize()
  _hold(f'level_leaf_render_extras n={n} B={B}', [(nm, out[:, k:k + 1], r64[:, k:k + 1], r32[:, k:k + 1], floor_fwd(n))
                                                  for k, nm in enumerate(['mean', 'p5', 'median', 'p95'])])
  if B > 8:
    assert out[0, 0].item() == t[0, -1].item()
    if n >= 3:
      assert out[4, 2].item() == t[4, n - 1].item()          # the median sits at the right-most fence-post of the flat run


@pytest.mark.parametrize('Cn', [1, 3])
@pytest.mark.parametrize('n,B', [(1, 3), (5, 65), (33, 17)])
def test_level_leaf_weighted_sum(ops, n, B, Cn):
  g = torch.Generator().manual_seed(1500 + n + Cn)
  w = torch.rand((B, n), generator=g)
  v = torch.randn((B, n, Cn), generator=g)
  r64, r32 = ((R.cast(w, dt)[..., None] * R.cast(v, dt)).sum(-2) for dt in (f64, f32))
  out = ops.weighted_sum(dev(w), dev(v))
  torch.cuda.synchronize()
  _hold(f'level_leaf_weighted_sum n={n} B={B} C={Cn}', [('sum', out, r64, r32, 2 * U if n == 1 else None)])


@pytest.mark.parametrize('with_offsets', [True, False])
def test_level_leaf_exposure_scale(ops, with_offsets):
  g = torch.Generator().manual_seed(1600)
  B, E = 70, 5
  ev = (0.1 + torch.rand(B, generator=g)).float()
  idx = torch.randint(-1, E, (B,), generator=g).to(torch.int32)       # -1 and 0: no offset
  assert (idx < 0).any() and (idx == 0).any() and (idx > 0).any()
  off = (torch.randn((E, 3), generator=g) * 0.1).float() if with_offsets else None
  r64, r32 = (R.exposure_scale(ev, idx, off, dt) for dt in (f64, f32))
  out = ops.exposure_scale(dev(ev), dev(idx), dev(off))
  torch.cuda.synchronize()
  _hold(f'level_leaf_exposure_scale offsets={with_offsets}', [('scale', out, r64, r32, 4 * U)])
  if not with_offsets:
    assert torch.equal(out.cpu(), ev[:, None].expand(B, 3))


# ----------------------------------------------------------------------------- the stand-alone loss kernels, long rays


@pytest.mark.parametrize('Bv', [64, 65])
def test_level_leaf_standalone_losses_128(ops, Bv):
  """mnr_interlevel_loss with a 128-bin histogram (98,816 B of LDS: the opt-in attribute path) and mnr_distortion_loss at 128
  samples, B = 130 with the valid rays ending at and one past a workgroup's 64; the per-element forms on the same input."""
  from oracle import stepfun as ostepfun
  n, ne, B = 128, 32, 130
  cfg, use = _cfg(2, 1, has_rgb=False)
  env = _inputs(1700, ne, B, cfg, use, 'bwd')
  hist = _histogram(1701, n, env)
  g = torch.Generator().manual_seed(1702)
  we = (torch.softmax(torch.randn((B, ne), generator=g) * 2, -1) * 0.3).float()    # (well below the histogram: w - w_outer does not cancel)
  t, w, te = hist['t_ref'], hist['w_ref'], env['sdist']

  def ref(dtype):
    c = lambda x: R.cast(x, dtype)
    wel, wl = c(we).requires_grad_(True), c(w).requires_grad_(True)
    li = R.interlevel_loss(1.0, c(t), c(w), c(te), wel, Bv)
    ld = R.distortion_loss(0.01, c(t), wl, Bv)
    (li + ld).backward()
    return dict(li=li.detach(), ld=ld.detach(), g_we=wel.grad, g_w=wl.grad, outer=ostepfun.lossfun_outer(c(t), c(w), c(te), c(we)),
                dist=ostepfun.lossfun_distortion(c(t), c(w)))

  r64, r32 = ref(f64), ref(f32)
  st = torch.zeros(2).cuda()
  g_we, g_w = torch.zeros((B, ne)).cuda(), torch.zeros((B, n)).cuda()
  ops.interlevel_loss(1.0, dev(t), dev(w), dev(te), dev(we), st[0:1], g_we, B_valid=Bv)
  ops.distortion_loss(0.01, dev(t), dev(w), st[1:2], g_w, B_valid=Bv)
  got = dict(li=st[0], ld=st[1], g_we=g_we, g_w=g_w, outer=ops.lossfun_outer(dev(t), dev(w), dev(te), dev(we)),
             dist=ops.lossfun_distortion(dev(t), dev(w)))
  torch.cuda.synchronize()
  _hold(f'level_leaf_standalone_losses_128 B_valid={Bv}', [(k, got[k], r64[k], r32[k], floor_scalar(n) if k in ('li', 'ld') else None) for k in got])
  assert torch.equal(g_we[Bv:].cpu(), torch.zeros((B - Bv, ne))) and torch.equal(g_w[Bv:].cpu(), torch.zeros((B - Bv, n)))


# ----------------------------------------------------------------------------- refusals


def test_level_leaf_refusals(ops):
  """What the launchers refuse before any launch: each is a ValueError and leaves the outputs alone."""
  L = ops.L
  B, n = 4, 5
  cfg, use = _cfg(2, 0)
  inp = _inputs(1800, n, B, cfg, use, 'bwd')
  c, a, kw, fwd = _kernel_forward(ops, cfg, inp)
  z = lambda *s: torch.zeros(s).cuda()
  for bad_n in (0, 1025):
    cb = ops.composite_cfg(bad_n, **cfg)
    m = max(bad_n, 1)                                  # (the tensors are real; the launchers refuse cfg.n)
    with pytest.raises(ValueError, match='n out of range'):
      ops.composite_fwd(cb, z(B, m), z(B, m + 1), z(B, 3), raw_rgb=z(B, m, 3))
    with pytest.raises(ValueError, match='n out of range'):
      ops.composite_bwd(cb, z(B, m), z(B, m + 1), z(B, 3), z(B, m), raw_rgb=z(B, m, 3))
  cbg = ops.composite_cfg(n, **dict(cfg, bg_mode=1))
  with pytest.raises(ValueError, match='bg'):
    ops.composite_fwd(cbg, *a, raw_rgb=kw['raw_rgb'])
  with pytest.raises(ValueError, match='bg'):
    ops.composite_bwd(cbg, *a, fwd['weights'], raw_rgb=kw['raw_rgb'], g_weights=z(B, n))
  wspec = dict(mode='distortion', mult=0.01, sdist=dev(inp['sdist']), stat=z(1))
  with pytest.raises(ValueError, match='mnr_level_bwd: null argument'):     # (the launcher's one message for B, B_valid and pointers)
    ops.composite_bwd(c, *a, fwd['weights'], **kw, losses=dict(B_valid=B + 1, data=None, weights=wspec))
  denom = torch.ones(1).cuda()
  with pytest.raises(ValueError, match='lossmult'):
    ops.composite_bwd(c, *a, fwd['weights'], **kw,
                      losses=dict(B_valid=B, weights=None, data=dict(type='mse', charb_padding=0.001, mult=1.0, rgb_out=fwd['rgb_out'],
                                                                     gt=z(B, 3), lossmult=z(B, 2), denom=denom, stats=z(2))))
  # the interlevel mode without t_ref, and a raydist_fn out of range: past the Python front ends, on the C structs
  g_rd = torch.full((B, n), 7.0).cuda()
  la = L.LevelBwdArgs()
  la.cfg, la.B, la.B_valid = c, B, B
  la.raw_density, la.tdist, la.dirs, la.weights = (t.data_ptr() for t in (a[0], a[1], a[2], fwd['weights']))
  la.raw_rgb, la.g_raw_density, la.data_loss_type = kw['raw_rgb'].data_ptr(), g_rd.data_ptr(), -1
  w_ref = z(B, 7)
  la.wloss_mode, la.wloss_mult, la.sdist, la.n_ref, la.w_ref = 1, 1.0, wspec['sdist'].data_ptr(), 7, w_ref.data_ptr()
  with pytest.raises(ValueError, match='t_ref'):
    L.check(ops.lib().mnr_level_bwd(C.byref(la), ops._stream()))
  sd, near, far, out = dev(inp['sdist']), torch.ones(B).cuda(), torch.full((B,), 2.0).cuda(), torch.full((B, n + 1), 7.0).cuda()
  sa = L.SdistBwdArgs()
  sa.B, sa.B_valid, sa.n = B, B, n
  sa.sdist, sa.near, sa.far, sa.g_sdist = sd.data_ptr(), near.data_ptr(), far.data_ptr(), out.data_ptr()
  for bad_fn in (-1, max(L.RAYDIST.values()) + 1):
    sa.raydist_fn = bad_fn
    with pytest.raises(ValueError, match='raydist_fn'):
      L.check(ops.lib().mnr_sdist_bwd(C.byref(sa), ops._stream()))
  with pytest.raises(ValueError, match='g_t0'):
    ops.sdist_bwd(sd, near, far, 'identity', g_t0=z(B, n), out=out)
  torch.cuda.synchronize()
  assert (g_rd == 7.0).all() and (out == 7.0).all()
