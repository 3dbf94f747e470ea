"""The oracle's Model / MLP composition against the reference's OWN models.py (tests/golden/models_*.npz).

tests/golden/make_golden_models.py executes reference internal/models.py (imported from where it lies, nothing copied)
on a NumPy float64 stand-in for jax.numpy with ~100 lines standing in for flax.linen / gin / jax.random, exact
complex-step derivatives for the Ref-NeRF normals, and logs every random draw.  Here the oracle gets the same
configuration, weights, rays and draws, in float64, and must reproduce every entry of `renderings` and `ray_history` of
every level: deterministic rendering and randomized training for 360 (contraction, dilation, annealing, GLO, density /
bottleneck noise, random background), blender_256, blender_refnerf (density-gradient normals, predicted normals, IDE,
tint, roughness, diffuse) and llff_raw (NDC cylinders, single MLP, exposure scaling, safe_exp colours).  The loss terms, clip_gradients and the
gradient of the total loss (directional derivatives through the reference's code) are held the same way.
"""

import importlib.util
import os

import numpy as np
import pytest
import torch

from multinerf_amd import configs, models, utils
from oracle import models as omodels
from tests import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_models', os.path.join(HERE, 'golden', 'make_golden_models.py'))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)
CASES = _gen.CASES
# Cases whose reference-side generator has a finite difference INSIDE the forward pass: density-gradient normals under the
# contraction (`refnerf_contract`: jax.linearize under the outer complex step of value_and_grad is a four-point real-axis stencil,
# tests/golden/make_golden_models.py `linearize`), whose 1e-12 error the sixteen IPE degrees' attenuation exp(-4^l var / 2)
# amplifies: measured 6e-9 relative in raw_grad_density, held to 5e-8.  Everything else is exact to rounding and held to 1e-9.
NESTED_FD = ('refnerf_contract',)
GOLD = _gen.load_gold()


def _sub(prefix):
  return {k[len(prefix):]: GOLD[k] for k in GOLD.files if k.startswith(prefix)}


def _tree(flat):
  tree = {}
  for k, v in flat.items():
    node = tree
    parts = k.split('/')
    for p in parts[:-1]:
      node = node.setdefault(p, {})
    node[parts[-1]] = torch.as_tensor(v.astype(np.float64))
  return tree


def _noise_from_log(case, B):
  """The reference's draws, in call order (models.py:190-191 jitter, :461-464 density noise, :531-533 bottleneck
  noise, :247-254 background), sorted into the oracle's explicit noise dict."""
  log = sorted(_sub(f'{case}/noise/').items())
  if not log:
    return None
  noise = {'u_jitter': {}, 'density_noise': {}, 'bottleneck_noise': {}, 'bg_rgbs': {}}
  level = -1
  for name, arr in log:
    t = torch.as_tensor(arr)
    if name.endswith('uniform') and not (arr.ndim == 2 and arr.shape[-1] == 3):
      level += 1
      noise['u_jitter'][level] = t
    elif name.endswith('uniform'):
      noise['bg_rgbs'][level] = t
    elif arr.ndim == 0:
      # drawn inside vmap(value_and_grad(predict_density)) (density-gradient normals): one value for the whole batch
      noise['density_noise'][level] = t.reshape(1, 1)
    elif arr.ndim == 2:
      noise['density_noise'][level] = t
    else:
      noise['bottleneck_noise'][level] = t
  return noise


@pytest.mark.parametrize('case', list(CASES))
def test_model_apply_matches_the_reference_source(case):
  preset, extra, B, randomized, train_frac = CASES[case]
  cfg = configs.load_preset(preset, list(extra))
  m = models.Model(config=cfg)
  om, on, op = helpers.oracle_hparams(m)
  params = _tree(_sub(f'{case}/param/'))
  r = _sub(f'{case}/rays/')
  f = lambda k: torch.as_tensor(r[k]) if k in r else None
  rays = utils.Rays(origins=f('origins'), directions=f('directions'), viewdirs=f('viewdirs'), radii=f('radii'),
                    imageplane=f('imageplane'), lossmult=f('lossmult'), near=f('near'), far=f('far'), cam_idx=f('cam_idx'),
                    exposure_idx=f('exposure_idx'), exposure_values=f('exposure_values'))
  noise = _noise_from_log(case, B)
  assert (noise is not None) == randomized
  rend, hist = omodels.model_apply(om, on, op, params, rays, float(GOLD[f'{case}/train_frac']), True, zero_glo=False, noise=noise)
  assert len(rend) == m.num_levels
  tol = dict(rtol=1e-9, atol=1e-11)
  if case in NESTED_FD:
    tol = dict(rtol=5e-8, atol=1e-10)
  checked = 0
  for lvl in range(m.num_levels):
    for group, got in (('rendering', rend[lvl]), ('history', hist[lvl])):
      want = _sub(f'{case}/{group}{lvl}/')
      assert want, (case, group, lvl)
      for k, w in want.items():
        assert k in got and got[k] is not None, (case, group, lvl, k)
        g = got[k].detach().numpy()
        assert g.shape == w.shape, (case, group, lvl, k, g.shape, w.shape)
        np.testing.assert_allclose(g, w, err_msg=f'{case} {group}{lvl} {k}', **tol)
        checked += 1
      # and nothing the reference leaves as None is produced by the oracle
      for k, v in got.items():
        if k not in want and k != 'tdist':
          assert v is None, (case, group, lvl, k)
  assert checked >= 12 * m.num_levels


@pytest.mark.parametrize('case', list(CASES))
def test_loss_terms_match_the_reference_source(case):
  """train_utils.py:72-197 executed by the generator on the reference's outputs; the oracle's on the oracle's."""
  from oracle import train_utils as otrain
  preset, extra, B, randomized, train_frac = CASES[case]
  cfg = configs.load_preset(preset, list(extra))
  m = models.Model(config=cfg)
  om, on, op = helpers.oracle_hparams(m)
  params = _tree(_sub(f'{case}/param/'))
  r = _sub(f'{case}/rays/')
  f = lambda k: torch.as_tensor(r[k]) if k in r else None
  rays = utils.Rays(origins=f('origins'), directions=f('directions'), viewdirs=f('viewdirs'), radii=f('radii'),
                    imageplane=f('imageplane'), lossmult=f('lossmult'), near=f('near'), far=f('far'), cam_idx=f('cam_idx'),
                    exposure_idx=f('exposure_idx'), exposure_values=f('exposure_values'))
  rend, hist = omodels.model_apply(om, on, op, params, rays, float(GOLD[f'{case}/train_frac']), True, zero_glo=False,
                                   noise=_noise_from_log(case, B))
  b = _sub(f'{case}/batch/')
  batch = utils.Batch(rays=rays, rgb=torch.as_tensor(b['rgb']), disps=torch.as_tensor(b['disps']),
                      alphas=torch.as_tensor(b['alphas']), normals=torch.as_tensor(b['normals']))
  want = _sub(f'{case}/loss/')
  tol = dict(rtol=1e-9, atol=1e-12)
  if case in NESTED_FD:
    tol = dict(rtol=5e-8, atol=1e-10)
  loss, stats = otrain.compute_data_loss(batch, rend, rays, cfg)
  np.testing.assert_allclose(float(loss.detach()), want["data"], **tol)
  assert {f'stats_{k}' for k in stats} == {k for k in want if k.startswith('stats_')}
  for k, v in stats.items():
    np.testing.assert_allclose(v.detach().numpy(), want[f"stats_{k}"], err_msg=k, **tol)
  np.testing.assert_allclose(float(torch.as_tensor(otrain.interlevel_loss(hist, cfg)).detach()), want['interlevel'], **tol)
  np.testing.assert_allclose(float(torch.as_tensor(otrain.distortion_loss(hist, cfg)).detach()), want['distortion'], **tol)
  if 'orientation' in want:
    np.testing.assert_allclose(float(otrain.orientation_loss(rays, om, hist, cfg).detach()), want['orientation'], **tol)
  if 'predicted_normal' in want:
    np.testing.assert_allclose(float(otrain.predicted_normal_loss(om, hist, cfg).detach()), want['predicted_normal'], **tol)
  assert ('orientation' in want) == (hist[-1][cfg.orientation_loss_target] is not None)
  # clip_gradients: per top-level module, by value then by norm (train_utils.py:200-218)
  grads = _tree(_sub(f'{case}/grad/'))
  clipped = otrain.clip_gradients(grads, cfg)
  changed = 0
  for name, w in _sub(f'{case}/clipped/').items():
    node = clipped
    for part in name.split('/'):
      node = node[part]
    np.testing.assert_allclose(node.numpy(), w, err_msg=name, rtol=1e-12, atol=0)
    changed += int(not np.array_equal(w, GOLD[f'{case}/grad/{name}']))
  assert changed > 0                                       # the clip did bite somewhere


def _direction(params_flat, rs):
  """The generator's seeded direction (make_golden_models.py: drawn over the sorted flat names, float32 values)."""
  out = {}
  for k in sorted(params_flat):
    v = params_flat[k].astype(np.float64)
    out[k] = (rs.normal(0, 1, v.shape) * (np.abs(v).mean() + 1e-3)).astype(np.float32).astype(np.float64)
  return out


@pytest.mark.parametrize('case', list(CASES))
def test_gradient_matches_the_reference_forward_differentiated(case):
  """d(total loss)/d(parameters) along three seeded directions.  Golden: complex-step differentiation THROUGH the
  reference's own models.py + train_utils.py with stop_gradient = "drop the perturbation" (for Ref-NeRF, whose forward
  already uses the complex step, a 4-point central difference with the stop_gradient values replayed).  Here: the
  oracle's autograd gradient of `train_utils.loss_fn` dotted with the same directions.  This pins where gradients flow
  (stop_level_grad, the interlevel loss's detached targets, RawNeRF's detached scaling) as well as the arithmetic."""
  from oracle import train_utils as otrain
  preset, extra, B, randomized, train_frac = CASES[case]
  cfg = configs.load_preset(preset, list(extra))
  cfg.compute_disp_metrics = cfg.compute_normal_metrics = False        # metrics never enter the loss
  cfg.randomized = randomized
  m = models.Model(config=cfg)
  om, on, op = helpers.oracle_hparams(m)
  flat = _sub(f'{case}/param/')
  params = _tree(flat)
  leaves = []
  def req(t):
    for k, v in t.items():
      if isinstance(v, dict):
        req(v)
      else:
        t[k] = v.clone().requires_grad_(True)
        leaves.append(t[k])
  req(params)
  r = _sub(f'{case}/rays/')
  f = lambda k: torch.as_tensor(r[k]) if k in r else None
  rays = utils.Rays(origins=f('origins'), directions=f('directions'), viewdirs=f('viewdirs'), radii=f('radii'),
                    imageplane=f('imageplane'), lossmult=f('lossmult'), near=f('near'), far=f('far'), cam_idx=f('cam_idx'),
                    exposure_idx=f('exposure_idx'), exposure_values=f('exposure_values'))
  b = _sub(f'{case}/batch/')
  batch = utils.Batch(rays=rays, rgb=torch.as_tensor(b['rgb']), disps=torch.as_tensor(b['disps']),
                      alphas=torch.as_tensor(b['alphas']), normals=torch.as_tensor(b['normals']))
  loss, _, _ = otrain.loss_fn(params, om, on, op, cfg, batch, float(GOLD[f'{case}/train_frac']), _noise_from_log(case, B))
  loss.backward()
  grads = {}
  def collect(t, prefix=''):
    for k, v in t.items():
      if isinstance(v, dict):
        collect(v, f'{prefix}{k}/')
      else:
        grads[f'{prefix}{k}'] = torch.zeros_like(v) if v.grad is None else v.grad
  collect(params)
  rs = np.random.RandomState(int(GOLD[f'{case}/seed']) + 3)
  # (the 4-point central difference of the generator where the forward pass is a complex step itself, density-gradient normals, or computes with complex numbers, the IDE)
  tol = 2e-5 if (not on.disable_density_normals or on.use_directional_enc) else 1e-8
  for d in range(3):
    V = _direction(flat, rs)
    got = sum(float((grads[k] * torch.as_tensor(V[k])).sum()) for k in V)
    want = float(GOLD[f'{case}/dloss{d}'])
    assert abs(got - want) <= tol * max(1.0, abs(want)), (case, d, got, want)
