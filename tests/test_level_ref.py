"""tests/level_ref.py on the CPU: the fp64 restatement the level leaf tests (tests/test_gpu_level_leaf.py) hold the kernels to
is the oracle's own arithmetic, and the inputs those tests plant give it finite, repeatable values."""

import pytest
import torch

from oracle import render as orender
from oracle import stepfun as ostepfun
from tests import level_ref as R
from tests import test_gpu_level_leaf as T

f64, f32 = torch.float64, torch.float32


@pytest.mark.parametrize('dtype', [f64, f32])
def test_alpha_weights_are_the_oracles(dtype):
  """forward() spells compute_alpha_weights and the first lines of volumetric_rendering out (to keep x = density * delta for
  d / d x, and to sum along the ray term by term in float32): in float64 bit for bit the oracle's, in float32 the oracle's up to
  the order of the sums."""
  for k, opaque in ((2, 0), (3, 1)):
    cfg, use = T._cfg(k, opaque ^ (k & 1))
    inp = T._inputs(7, 33, 9, cfg, use, 'fwd')
    _, f = T._ref_forward(cfg, inp, dtype)
    c = lambda key: R.cast(inp[key], dtype)
    w, _, _ = orender.compute_alpha_weights(f['density'], c('tdist'), c('dirs'), opaque_background=cfg['opaque_background'])
    bg = c('bg') if cfg['bg_mode'] == 1 else cfg['bg_value']
    rgb = orender.volumetric_rendering(f['rgb'], w, c('tdist'), bg, c('tdist')[:, -1:], False)['rgb']
    if dtype == f64:
      assert torch.equal(w, f['weights']) and torch.equal(rgb, f['rgb_out'])
    else:
      torch.testing.assert_close(f['weights'], w, rtol=2e-5, atol=1e-7)
      torch.testing.assert_close(f['rgb_out'], rgb, rtol=2e-5, atol=1e-6)


def test_float32_sums_along_the_ray_are_term_by_term():
  import numpy as np
  x = torch.rand((3, 1000), generator=torch.Generator().manual_seed(1))
  want = torch.from_numpy(np.cumsum(x.numpy(), axis=-1, dtype=np.float32))
  assert torch.equal(R.cumsum_ray(x), want) and torch.equal(R.sum_ray(x), want[:, -1])
  assert torch.equal(R.cumsum_ray(x.double()), torch.cumsum(x.double(), -1))


def test_activation_derivatives():
  x = torch.tensor([-3.0, -0.5, 0.0, 0.7, 90.0], dtype=f64, requires_grad=True)
  want = {'sigmoid': lambda y: y * (1 - y), 'safe_exp': lambda y: y, 'softplus': lambda y: torch.sigmoid(x.detach()),
          'exp': lambda y: y, 'relu': lambda y: (x.detach() > 0).double(), 'identity': lambda y: torch.ones_like(y)}
  assert set(want) == set(R.ACTS)
  for kind in R.ACTS:
    y = R.act(kind, x)
    g, = torch.autograd.grad(y.sum(), x)
    torch.testing.assert_close(g, want[kind](y.detach()), rtol=1e-14, atol=0)
  assert R.act('safe_exp', x)[-1].item() == torch.exp(torch.tensor(88.0, dtype=f64)).item()


@pytest.mark.parametrize('row', T.FWD_ROWS, ids=T._row_id)
def test_planted_forward_rays_are_finite_and_repeatable(row):
  (n, B), form, k, flip = row
  cfg, use = T._cfg(k, flip)
  runs = []
  for _ in range(2):
    inp = T._inputs(100 + k, n, B, cfg, use, 'fwd')
    _, f = T._ref_forward(cfg, inp, f64)
    runs.append(f)
  for nm in ('density', 'weights', 'rgb_out', 'acc') + (('rgb',) if cfg['has_rgb'] else ()):
    assert torch.isfinite(runs[0][nm]).all(), nm
    assert torch.equal(runs[0][nm], runs[1][nm]), nm
  w = runs[0]['weights']
  if not (cfg['opaque_background'] and min(1, n - 1) == n - 1):
    assert w[0, min(1, n - 1)] == 0                                    # the zero-width interval
  if B > 1:
    assert (w[1, :n - 1] == 0).all()                                   # the zero direction vector
  if B > 2 and n > 3 and cfg['density_act'] != 'sigmoid':
    assert w[2, 3:].abs().max() < 1e-40                                # behind the saturated sample


@pytest.mark.parametrize('shape', T.INTERLEVEL, ids=lambda s: f'n{s[0][0]}-nref{s[0][1]}')
def test_planted_histograms(shape):
  """The inputs of test_level_leaf_bwd_interlevel themselves (its seeds and configuration)."""
  (n, n_ref), B = shape
  i = T.INTERLEVEL.index(shape)
  cfg, use = T._cfg(2, i % 2, has_rgb=(n == 128))
  inp = T._inputs(800 + i, n, B, cfg, use, 'bwd')
  h = T._histogram(900 + i, n_ref, inp)
  t, w, sd = h['t_ref'], h['w_ref'], inp['sdist']
  assert (t[:, 1:] >= t[:, :-1]).all() and (sd[:, 1:] >= sd[:, :-1]).all()
  assert (w == 0).any()
  below, above = t[:, 0] < sd[:, 0], t[:, -1] > sd[:, -1]
  assert (below & above).any()                                         # reaches below and above the envelope
  assert ((t[:, 0] >= 0.2) & (t[:, -1] <= 0.7)).any()                  # lies inside it
  assert (sd[0, 1:] == sd[0, :-1]).any()                               # a zero-width interval of the envelope
  if n_ref >= 2:
    assert (t[3, 1:] == t[3, :-1]).any()                               # ... and of the histogram, after the sort
  if n >= 2 and n_ref >= 2:
    assert (t[:, 1:-1, None] == sd[:, None, 1:-1]).any()               # an interior tie
  for dtype in (f64, f32):
    twice = []
    for _ in range(2):
      _, f = T._ref_forward(cfg, inp, dtype)
      twice.append(ostepfun.lossfun_outer(R.cast(t, dtype), R.cast(w, dtype), R.cast(sd, dtype), f['weights']))
    assert torch.isfinite(twice[0]).all() and torch.equal(twice[0], twice[1])


@pytest.mark.parametrize('fn', R.RAYDISTS, ids=str)
def test_ray_warps_are_defined_on_the_test_ranges(fn):
  lo, hi = T.NEAR_FAR[fn]
  s = torch.linspace(0, 1, 11, dtype=f64)[None].requires_grad_(True)
  near, far = torch.tensor([lo], dtype=f64), torch.tensor([hi + 1.0], dtype=f64)
  t = R.s_to_t(fn, s, near, far)
  g, = torch.autograd.grad(t.sum(), s)
  assert torch.isfinite(t).all() and torch.isfinite(g).all() and (g > 0).all()
  torch.testing.assert_close(t[0, [0, -1]], torch.cat([near, far]), rtol=1e-12, atol=0)
  if fn == 'piecewise':
    assert t.min() < 1 < t.max()
