"""Oracle Model/MLP/train_step: architecture goldens + self-consistency (CPU).

(The composition itself is pinned against the reference's own source in
tests/test_oracle_models_golden.py.)  Pinned here: the parameter counts published in the
reference's scripts/generate_tables.ipynb (:145, :340/:344, :684, :1050), the
flax tree naming, output shapes, and train_step mechanics (Adam == torch.optim.Adam
with optax's epsilon placement, clipping, finite gradients at train_frac = 0).
"""

import numpy as np
import pytest
import torch

from multinerf_amd import configs, models
from oracle import models as omodels
from oracle import train_utils as otrain
from tests import helpers

PUBLISHED = {'360': 9007493, 'blender_256': 835205, 'blender_refnerf': 713230, 'llff_raw': 615740}
PUBLISHED_FILES = {'blender_512.gin': 3065733, 'llff_512.gin': 3065733, 'llff_256.gin': 835205}     # generate_tables.ipynb:349


@pytest.mark.parametrize('name', list(PUBLISHED))
def test_param_counts_match_published(name):
  cfg = configs.load_preset(name)
  m = models.Model(config=cfg)
  om, on, op = helpers.oracle_hparams(m)
  params = omodels.init_params(om, on, op)
  assert omodels.param_count(params) == PUBLISHED[name]
  assert list(params)[0] == 'NerfMLP_0'                       # construction order, models.py:98-99
  if True:
    m.build('cpu')
    assert m.num_params == PUBLISHED[name]                    # product layout agrees
    tree = m.params_tree(torch.zeros(m.num_params))
    for mod in params:
      assert list(tree[mod]) == list(params[mod])
      for dn in params[mod]:
        if dn == 'embedding':
          assert tree[mod][dn].shape == params[mod][dn].shape
        else:
          assert tree[mod][dn]['kernel'].shape == params[mod][dn]['kernel'].shape


@pytest.mark.parametrize('fname', list(PUBLISHED_FILES))
def test_param_counts_of_the_other_reference_configs(fname):
  """Bound as the reference's own gin files bind (recorded in tests/golden/reference_gin_bindings.json)."""
  from multinerf_amd import gin
  gin.clear_config()
  gin._BINDINGS.update(helpers.reference_gin_bindings(fname[:-len('.gin')]))
  cfg = configs.load_config([], [])
  m = models.Model(config=cfg)
  om, on, op = helpers.oracle_hparams(m)
  assert omodels.param_count(omodels.init_params(om, on, op)) == PUBLISHED_FILES[fname]
  m.build('cpu')
  assert m.num_params == PUBLISHED_FILES[fname]
  gin.clear_config()


def test_360_glo4_param_count():
  cfg = configs.load_preset('360', ['Model.num_glo_features = 4'])
  m = models.Model(config=cfg)
  om, on, op = helpers.oracle_hparams(m)
  params = omodels.init_params(om, on, op)
  assert omodels.param_count(params) == 9012005   # ipynb:155/164
  m.build('cpu')
  assert m.num_params == 9012005
  tree = m.params_tree(torch.zeros(m.num_params))
  assert tree['Embed_0']['embedding'].shape == params['Embed_0']['embedding'].shape == (1000, 4)


def _tiny(name, extra=()):
  cfg = configs.load_preset(name, list(extra))
  m = models.Model(config=cfg)
  return cfg, m, helpers.oracle_hparams(m)


@pytest.mark.parametrize('name,extra', [
    ('360', ['NerfMLP.net_width = 64', 'PropMLP.net_width = 32']),
    ('blender_256', ['NerfMLP.net_width = 32', 'PropMLP.net_width = 32']),
    ('blender_refnerf', ['NerfMLP.net_width = 32', 'NerfMLP.net_width_viewdirs = 16']),
    ('llff_raw', ['NerfMLP.net_width = 32']),
])
def test_forward_shapes_and_train_step(name, extra):
  cfg, m, (om, on, op) = _tiny(name, extra)
  B = 6
  near, far = cfg.near, cfg.far
  batch = helpers.synthetic_rays(B, near=max(near, 1e-3) if name != 'llff_raw' else 0., far=far)
  rays = batch.rays
  if name == 'llff_raw':
    rays.exposure_idx = torch.tensor([[0], [1], [2], [0], [3], [1]], dtype=torch.int64)
    rays.exposure_values = torch.full((B, 1), 0.7)
    rays.lossmult = torch.rand((B, 3))
  if name == 'blender_refnerf':
    batch.normals = torch.randn((B, 3))
    batch.alphas = torch.ones((B,))
  params = omodels.init_params(om, on, op, seed=1)
  noise = helpers.make_noise(m, B)
  rend, hist = omodels.model_apply(om, on, op, params, rays, 0.5, True, zero_glo=False, noise=noise)
  assert len(rend) == m.num_levels and len(hist) == m.num_levels
  n_last = m.num_nerf_samples
  assert rend[-1]['rgb'].shape == (B, 3) and hist[-1]['sdist'].shape == (B, n_last + 1)
  assert hist[-1]['weights'].shape == (B, n_last) and rend[-1]['distance_median'].shape == (B,)
  for r in rend:
    assert torch.isfinite(r['rgb']).all()
  if name == 'blender_refnerf':
    assert hist[-1]['normals'].shape == (B, n_last, 3) and hist[-1]['roughness'].shape == (B, n_last, 1)
  # one optimisation step; also at train_frac = 0 (anneal = 0 -> 0*log(w) edge, SURVEY hard part 8)
  for tf in (0.0, 0.5):
    st = otrain.init_opt_state(params)
    new_p, new_s, stats, grads = otrain.train_step(params, st, om, on, op, cfg, batch, tf, noise=noise)
    leaves = [g for _, g in otrain.tree_leaves(grads)]
    assert all(torch.isfinite(g).all() for g in leaves)
    assert any(g.abs().sum() > 0 for g in leaves)
    assert new_s['count'] == 1 and np.isfinite(float(stats['loss']))


def test_adam_matches_torch_adam():
  """optax.adam == torch Adam up to where eps enters (both: m_hat/(sqrt(v_hat)+eps))."""
  class C:
    adam_beta1, adam_beta2, adam_eps = 0.9, 0.999, 1e-6
    lr_init = lr_final = 1e-2
    max_steps, lr_delay_steps, lr_delay_mult = 100, 0, 1
  p0 = torch.randn(50, dtype=torch.float64)
  params = {'m': {'w': p0.clone()}}
  tp = p0.clone().requires_grad_(True)
  opt = torch.optim.Adam([tp], lr=1e-2, betas=(0.9, 0.999), eps=1e-6)
  st = otrain.init_opt_state(params)
  for i in range(5):
    g = torch.sin(torch.arange(50, dtype=torch.float64) * (i + 1))
    params, st = otrain.adam_update(params, {'m': {'w': g}}, st, C)
    tp.grad = g.clone()
    opt.step()
  np.testing.assert_allclose(params['m']['w'].numpy(), tp.detach().numpy(), rtol=1e-10, atol=1e-12)


def test_bf16_dense_emulation_is_close_to_fp32():
  cfg, m, (om, on, op) = _tiny('360', ['NerfMLP.net_width = 64', 'PropMLP.net_width = 32'])
  batch = helpers.synthetic_rays(8)
  params = omodels.init_params(om, on, op, seed=2)
  r32, _ = omodels.model_apply(om, on, op, params, batch.rays, 0.5, False)
  r16, _ = omodels.model_apply(om, on, op, params, batch.rays, 0.5, False, dense_dtype=torch.bfloat16)
  assert (r32[-1]['rgb'] - r16[-1]['rgb']).abs().max() < 0.05


def test_bf16_forward_and_backward_emulation_of_a_dense_layer():
  """oracle.models.BF16_FWD_BWD (the reference's TPU default precision in both passes of a Dense matmul): the forward is the
  forward-only emulation's, the backward multiplies the bf16-rounded incoming gradient with the bf16-rounded operands."""
  from oracle import models as om
  g = torch.Generator().manual_seed(0)
  x = torch.randn((6, 9), generator=g, requires_grad=True)
  k = torch.randn((9, 5), generator=g, requires_grad=True)
  b = torch.randn((5,), generator=g)
  gy = torch.randn((6, 5), generator=g)
  p = {'Dense_0': {'kernel': k, 'bias': b}}
  y_fb = om._DenseCursor(p, om.BF16_FWD_BWD)(x)
  y_f = om._DenseCursor(p, torch.bfloat16)(x)
  assert torch.equal(y_fb, y_f)
  y_fb.backward(gy)
  r = lambda t: t.detach().bfloat16().float()
  assert torch.equal(x.grad, r(gy) @ r(k).t()) and torch.equal(k.grad, r(x).t() @ r(gy))
  gx_fb = x.grad.clone()
  x.grad = k.grad = None
  y_f.backward(gy)
  assert not torch.equal(x.grad, gx_fb) and torch.allclose(x.grad, gx_fb, rtol=0, atol=0.05)      # (the incoming gradient unrounded)
