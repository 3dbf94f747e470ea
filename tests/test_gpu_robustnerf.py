"""RobustNeRF on the GPU (-m gpu): mnr_robustnerf_mask and mnr_quantile against the reference's own outputs
(tests/golden/robustnerf.npz, made by tests/golden/make_golden_robustnerf.py), and the composed train step of the
360_robustnerf preset at the reduced widths tests/test_gpu_model.py uses.

Bounds.  The fixture keeps every per-pixel error further than a relative 1e-5 from the threshold and every vote off its
tie, so the mask (and lossmult * mask) must match element for element.  The four means are ratios of integer counts and
the mse a sum the kernel accumulates in double per patch: 1e-6 relative, as the quantile (two exact order statistics and
one interpolation).  The composed cases are described at each test.
"""

import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import configs, models, ops, train_utils
from oracle import models as omodels
from oracle import train_utils as otrain
from tests import helpers
from tests import robustnerf_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'robustnerf.npz')
CASE_NAMES = ['preset', 'odd', 'f1', 'f5', 'disabled', 'q08', 'thr0', 'thrbig', 'padded']


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')


@pytest.fixture(scope='module')
def golden_cases():
  z = np.load(GOLDEN)
  names = sorted({k.split('/')[0] for k in z.files})
  assert names == sorted(CASE_NAMES)
  return {n: {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(n + '/')} for n in names}


def _dev(x):
  return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def _run_mask(g, **over):
  P, inner, f, B_valid, enable = (int(v) for v in g['params'])
  qs, qp, qi = (float(v) for v in g['quantiles'])
  rgb, gt, lm = _dev(g['rgb']), _dev(g['gt']), _dev(g['lossmult'])
  B = rgb.shape[0]
  thr = _dev(np.array([float(g['threshold'])]))
  denom = torch.zeros(1).cuda()
  ops.lossmult_sum(lm, B_valid, denom)
  stats, mse = torch.zeros(4).cuda(), torch.zeros(1).cuda()
  err = torch.full((B,), -1.0).cuda()
  kw = dict(B_valid=B_valid, patch_size=P, inner_patch_size=inner, filter_size=f, smoothed_inlier_quantile=qs,
            inner_patch_inlier_quantile=qp, enable=bool(enable), err=err, stats=stats, mse=mse, denom=denom)
  kw.update(over)
  mask, lm_out = ops.robustnerf_mask(rgb, gt, lm, thr, **kw)
  nxt = ops.quantile(err, qi, N=B_valid)
  torch.cuda.synchronize()
  return dict(mask=mask.cpu().numpy(), lm_out=lm_out.cpu().numpy(), stats=stats.cpu().numpy().astype(np.float64),
              mse=float(mse.cpu()[0]), err=err.cpu().numpy(), next=float(nxt.cpu()[0]), B_valid=B_valid)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_mask_kernel_equals_the_reference(golden_cases, name):
  g = golden_cases[name]
  out = _run_mask(g)
  B_valid = out['B_valid']
  mism = int((out['mask'] != g['mask']).sum())
  print(f'{name}: B {g["mask"].shape[0]} B_valid {B_valid} mask mismatches {mism}, mean mask {out["mask"][:B_valid].mean():.4f}')
  assert mism == 0
  assert np.array_equal(out['lm_out'].astype(np.float64), g['lossmult_masked'].reshape(out['lm_out'].shape))
  err64 = ref.per_pixel_error(g['rgb'][:B_valid], g['gt'][:B_valid])
  np.testing.assert_allclose(out['err'][:B_valid], err64, rtol=1e-6, atol=0)
  assert np.all(out['err'][B_valid:] == -1.0)                       # nothing is written behind B_valid
  for k, nm in enumerate(ref.STAT_NAMES):
    print(f'{name}: {nm} kernel {out["stats"][k]:.9g} reference {g["stats"][k]:.9g}')
  np.testing.assert_allclose(out['stats'], g['stats'], rtol=1e-6, atol=0)
  print(f'{name}: mse kernel {out["mse"]:.9g} reference {float(g["mse"]):.9g}; next threshold kernel {out["next"]:.9g} '
        f'reference {float(g["next_threshold"]):.9g}')
  assert abs(out['mse'] - float(g['mse'])) <= 1e-6 * float(g['mse'])
  assert abs(out['next'] - float(g['next_threshold'])) <= 1e-6 * float(g['next_threshold'])


def test_mask_kernel_optional_outputs_may_be_absent(golden_cases):
  g = golden_cases['odd']
  out = _run_mask(golden_cases['odd'], stats=None, mse=None, denom=None)
  assert np.array_equal(out['mask'], g['mask'])


@pytest.mark.parametrize('N', [1, 2, 255, 16384, 65536])
@pytest.mark.parametrize('q', [0.0, 0.5, 0.8, 1.0])
def test_quantile_equals_numpy(N, q):
  rs = np.random.RandomState(N + int(100 * q))
  x = (rs.standard_normal(N) ** 2 * 10.0 ** rs.uniform(-6, 0, N)).astype(np.float32)       # errors over six decades
  if N >= 255:
    x[rs.randint(0, N, N // 16)] = x[0]                                                      # repeated values
    x[rs.randint(0, N, 3)] = 0.0
  want = float(np.quantile(x.astype(np.float64), q))
  got = float(ops.quantile(torch.as_tensor(x).cuda(), q).cpu()[0])
  print(f'N {N} q {q}: kernel {got:.9g} numpy {want:.9g}')
  assert abs(got - want) <= 1e-6 * abs(want)
  # deterministic, and the same through a longer buffer with N given
  buf = torch.cat([torch.as_tensor(x), torch.full((5,), 1e9)]).cuda()
  assert float(ops.quantile(buf, q, N=N).cpu()[0]) == got


def test_quantile_ignores_non_finite_values():
  rs = np.random.RandomState(5)
  x = rs.uniform(0, 1, 1000).astype(np.float32)
  y = np.concatenate([x, np.array([np.inf, np.nan, np.inf], np.float32)])
  rs.shuffle(y)
  for q in (0.0, 0.3, 1.0):
    want = float(np.quantile(x.astype(np.float64), q))
    got = float(ops.quantile(torch.as_tensor(y).cuda(), q).cpu()[0])
    assert abs(got - want) <= 1e-6 * abs(want)
  assert np.isnan(float(ops.quantile(torch.full((7,), float('nan')).cuda(), 0.5).cpu()[0]))


def test_argument_errors_are_raised_not_launched(golden_cases):
  g = golden_cases['odd']                                             # P = 8, 32 patches
  with pytest.raises(ValueError, match='1024'):
    _run_mask(dict(g, params=np.array([33, 8, 3, 33 * 33, 1])))
  with pytest.raises(ValueError, match='odd and at most patch_size'):
    _run_mask(g, filter_size=4)
  with pytest.raises(ValueError, match='odd and at most patch_size'):
    _run_mask(g, filter_size=9)
  with pytest.raises(ValueError, match='at most patch_size'):
    _run_mask(g, inner_patch_size=9)
  with pytest.raises(ValueError, match='multiple of patch_size'):
    _run_mask(g, B_valid=8 * 8 * 3 + 5)
  with pytest.raises(ValueError, match='bad batch sizes|must match the batch'):
    _run_mask(g, B_valid=64 * 33)
  with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
    ops.quantile(torch.zeros(4).cuda(), 1.5)
  with pytest.raises(ValueError, match='exceeds'):
    ops.quantile(torch.zeros(4).cuda(), 0.5, N=5)
  cfg = configs.load_preset('360_robustnerf', WIDTHS + ['Config.robustnerf_inner_patch_size = 17'])
  model = models.Model(config=cfg)
  model.build('cuda')
  with pytest.raises(ValueError, match='robustnerf_inner_patch_size'):
    train_utils.create_train_step(model, cfg)


# ----------------------------------------------------------------------------- composed: the train step of the new preset

WIDTHS = ['NerfMLP.net_width = 256', 'PropMLP.net_width = 128']      # the reduced widths of tests/test_gpu_model.py's 360 cases
B_RAYS = 512                                                          # two 16 x 16 patches


def _setup(extra=(), seed=3, patch=16):
  """tests/test_gpu_model.py's _setup on the new preset, with rays laid out as patches and a ground truth that has
  spatial structure: a smooth image per patch with a bright square painted into one of them (a distractor)."""
  cfg = configs.load_preset('360_robustnerf', WIDTHS + list(extra))
  model = models.Model(config=cfg)
  model.build('cuda')
  om, on, op = helpers.oracle_hparams(model)
  params = omodels.init_params(om, on, op, seed=seed)
  g = torch.Generator().manual_seed(seed + 1)
  for mname, mod in params.items():
    if mname in ('exposure_scaling_offsets', 'Embed_0'):
      continue
    for d in mod.values():
      d['bias'] = 0.05 * torch.randn(d['bias'].shape, generator=g)
  batch = helpers.synthetic_rays(B_RAYS, near=cfg.near, far=cfg.far)
  P = patch
  yy, xx = np.meshgrid(np.arange(P), np.arange(P), indexing='ij')
  img = np.zeros((B_RAYS // (P * P), P, P, 3), np.float32)
  for p in range(img.shape[0]):
    for ch in range(3):
      img[p, ..., ch] = 0.5 + 0.3 * np.sin(0.3 * xx * (ch + 1) + 0.2 * yy + p)
  img[0, 3:9, 5:12] = 1.0
  batch.rgb = torch.as_tensor(img.reshape(-1, 3))
  batch.rays.lossmult = (0.5 + torch.rand((B_RAYS, 1), generator=g)).float()
  flat = model.flat_from_tree(params)
  return cfg, model, (om, on, op), params, flat, batch


def _step(cfg, model, flat, batch, thr, noise, state=None):
  if state is None:
    state, _ = train_utils.create_optimizer(cfg, {'flat': flat.clone(), 'params': None})
  step = train_utils.create_train_step(model, cfg)
  state2, stats, _ = step(0, state, batch.map(lambda t: t.cuda()), None, 0.3, thr, noise=noise, return_grads=True)
  torch.cuda.synchronize()
  return state2, stats


def _mask_kw(cfg, B_valid):
  return dict(B_valid=B_valid, patch_size=cfg.patch_size, inner_patch_size=cfg.robustnerf_inner_patch_size,
              filter_size=cfg.robustnerf_smoothed_filter_size, smoothed_inlier_quantile=cfg.robustnerf_smoothed_inlier_quantile,
              inner_patch_inlier_quantile=cfg.robustnerf_inner_patch_inlier_quantile, enable=cfg.enable_robustnerf_loss)


# Two steps on the device never agree bit for bit, even two runs of the SAME configuration: the weight-gradient GEMMs and the
# statistics accumulate with fp32 atomics whose arrival order changes from run to run.  tests/test_gpu_model.py holds two
# gradients that are equal "up to the arrival order of the fp32 atomics" to a relative 1e-4 per module
# (test_side_stream_equals_one_stream_when_both_mlps_share_a_workspace_shape); the same bound is used here.  So the two
# equalities below are asserted bit for bit where the arithmetic is ordered -- what the unchanged level kernels are HANDED,
# and the whole step on the sequentially consistent simulator -- and on the device at that 1e-4, with the run-to-run distance
# of the twin printed next to it (measured on the MI355X, profiles/robustnerf.md: twin against itself up to 9.5e-6, robustnerf
# against the twin 1.4e-7 to 2.0e-7).
ORDERED = os.environ.get('MNR_TESTS_ON_SIMULATOR') == '1'
ATOMIC_ORDER_TOL = 1e-4


def _same_gradient(model, g, g_twin, g_twin_again, what):
  for mod, b, e in model.modules:
    r = g_twin[b:e].double()
    d = ((g[b:e].double() - r).norm() / (r.norm() + 1e-30)).item()
    floor = ((g_twin_again[b:e].double() - r).norm() / (r.norm() + 1e-30)).item()
    print(f'{what} {mod}: |g - g_twin| / |g_twin| = {d:.3e}; the twin run twice: {floor:.3e}')
    assert d <= ATOMIC_ORDER_TOL, (mod, d)
  if ORDERED:
    assert torch.equal(g, g_twin)


def test_huge_threshold_is_the_mse_step():
  """loss_threshold = 1e30: every pixel is an inlier, lossmult * mask IS lossmult (bit for bit), and the level kernels run the
  same MSE branch on the same numbers as data_loss_type = 'mse': the same gradients and the same statistics (see ORDERED above
  for "the same" on a device with fp32 atomics).  The logged mse entries come from mnr_robustnerf_mask in this mode (the level
  kernels report the masked mse): the same terms in another order, 1e-6 relative."""
  cfg, model, _, _, flat, batch = _setup()
  noise = helpers.make_noise(model, B_RAYS)
  cfg_mse = dataclasses.replace(cfg, data_loss_type='mse')
  _, s_mse = _step(cfg_mse, model, flat, batch, 1.0, noise)
  _, s_mse2 = _step(cfg_mse, model, flat, batch, 1.0, noise)
  _, s_rob = _step(cfg, model, flat, batch, 1e30, noise)
  rb = model._saved['robust']
  assert torch.all(rb['mask'][-1][:B_RAYS] == 1)
  assert torch.equal(rb['lossmult'][-1][:B_RAYS], model._saved['rays'].lossmult[:B_RAYS])     # what the level kernel is handed
  _same_gradient(model, s_rob['_grads'], s_mse['_grads'], s_mse2['_grads'], 'threshold 1e30 vs mse:')
  raw_m, raw_r = s_mse['_raw'].cpu().numpy().astype(np.float64), s_rob['_raw'].cpu().numpy().astype(np.float64)
  n = s_mse['_nlev']
  assert raw_r.shape[0] == raw_m.shape[0] + 5
  mse_idx = list(range(0, 2 * n, 2))
  rest = [i for i in range(raw_m.shape[0]) if i not in mse_idx]
  print('statistics, mse step:', raw_m, 'robustnerf step:', raw_r)
  if ORDERED:
    assert np.array_equal(raw_r[rest], raw_m[rest])
    assert torch.equal(s_rob['grad_sqnorms'], s_mse['grad_sqnorms'])
  np.testing.assert_allclose(raw_r[rest], raw_m[rest], rtol=1e-6, atol=0)
  np.testing.assert_allclose(raw_r[mse_idx], raw_m[mse_idx], rtol=1e-6, atol=0)
  m = s_rob.materialize()
  assert m['mask'] == 1.0 and m['is_inlier_loss'] == 1.0 and m['loss_threshold'] > 0


def test_zero_threshold_masks_the_data_loss_out():
  """loss_threshold = 0: no error is below it, the box votes are 0 and the patch votes are 0: a zero mask, lossmult * mask = 0
  bit for bit, a zero data loss, and the gradient of the step with both data-loss multipliers 0 (see ORDERED above)."""
  cfg, model, _, _, flat, batch = _setup()
  noise = helpers.make_noise(model, B_RAYS)
  cfg_off = dataclasses.replace(cfg, data_loss_type='mse', data_loss_mult=0.0, data_coarse_loss_mult=0.0)
  _, s_off = _step(cfg_off, model, flat, batch, 1.0, noise)
  _, s_off2 = _step(cfg_off, model, flat, batch, 1.0, noise)
  _, s_rob = _step(cfg, model, flat, batch, 0.0, noise)
  m = s_rob.materialize()
  assert m['losses']['data'] == 0.0 and m['mask'] == 0.0 and m['is_inlier_loss'] == 0.0 and m['is_inlier_patch'] == 0.0
  assert torch.all(model._saved['robust']['mask'][-1] == 0) and torch.all(model._saved['robust']['lossmult'][-1] == 0)
  _same_gradient(model, s_rob['_grads'], s_off['_grads'], s_off2['_grads'], 'threshold 0 vs no data loss:')
  assert s_rob['_grads'].abs().max() > 0                              # (interlevel and distortion are still there)


def test_mid_threshold_mask_loss_and_gradient():
  """A threshold taken from a first step's own quantile, then a step with it (interlevel and distortion off, so that the data
  loss is the whole gradient).  The mask equals the float64 restatement's on the step's own rendered rgb; the data-loss statistic
  agrees at 1e-5; the gradient is sum(lossmult * mask) / sum(lossmult) times the oracle's MSE gradient under lossmult * mask
  (its denominator is sum(lossmult * mask)), within the per-module tolerances tests/test_gpu_model.py applies to 360."""
  from tests.test_gpu_model import TOL, TOL32
  extra = ['Config.interlevel_loss_mult = 0.0', 'Config.distortion_loss_mult = 0.0']
  cfg, model, (om, on, op), params, flat, batch = _setup(extra)
  noise = helpers.make_noise(model, B_RAYS)
  _, s0 = _step(cfg, model, flat, batch, 1.0, noise)
  thr_dev = s0.loss_threshold_device()
  assert thr_dev.dim() == 0 and thr_dev.device == s0['_raw'].device
  thr = float(thr_dev.cpu())
  # the same parameters again (the first step's Adam update went into a copy), now under the quantile of its own errors
  _, s1 = _step(cfg, model, flat, batch, thr_dev, noise)
  rb = model._saved['robust']
  rgb = model._saved['levels'][-1]['rgb_out'][:B_RAYS].cpu().numpy()
  gt = batch.rgb.numpy()
  lm = batch.rays.lossmult.numpy().astype(np.float64)
  want = ref.robustnerf_mask_f64(rgb, gt, thr, **_mask_kw(cfg, B_RAYS))
  margin = np.min(np.abs(want['err'] - thr) / thr)
  got_mask = rb['mask'][-1][:B_RAYS].cpu().numpy()
  print(f'threshold {thr:.6g} (q = {cfg.robustnerf_inlier_quantile}), closest error at a relative {margin:.3g}, mask mean {got_mask.mean():.4f}, '
        f'criteria alone: {[int((want["parts"][k] & ~np.any([want["parts"][j] for j in want["parts"] if j != k], 0)).sum()) for k in want["parts"]]}')
  assert np.array_equal(got_mask, want['mask'])
  assert 0.0 < got_mask.mean() < 1.0
  m = s1.materialize()
  for k in ref.STAT_NAMES:
    assert abs(m[k] - want['stats'][k]) <= 1e-6 * want['stats'][k] + 1e-12, k
  d = rgb.astype(np.float64) - gt
  data64 = float((lm * want['mask'][:, None] * d * d).sum() / (3 * lm.sum()))
  print(f'data loss kernel {m["losses"]["data"]:.9g} float64 {data64:.9g}; mse kernel {m["mses"][-1]:.9g} float64 {ref.weighted_mse(rgb, gt, lm, B_RAYS):.9g}')
  assert abs(m['losses']['data'] - data64) <= 1e-5 * data64
  assert abs(m['mses'][-1] - ref.weighted_mse(rgb, gt, lm, B_RAYS)) <= 1e-5 * m['mses'][-1]
  assert abs(m['loss_threshold'] - np.quantile(want['err'], cfg.robustnerf_inlier_quantile)) <= 1e-6 * m['loss_threshold']
  # gradient: the oracle's MSE step with lossmult * mask, rescaled to the unmasked denominator
  cfg_o = dataclasses.replace(cfg, data_loss_type='mse')
  batch_o = dataclasses.replace(batch, rays=dataclasses.replace(batch.rays, lossmult=torch.as_tensor(lm * want['mask'][:, None], dtype=torch.float32)))
  scale = float((lm * want['mask'][:, None]).sum() / lm.sum())
  st = otrain.init_opt_state(params)
  _, _, _, g_o = otrain.train_step(params, st, om, on, op, cfg_o, batch_o, 0.3, noise=noise, dense_dtype=torch.bfloat16)
  _, _, _, g_32 = otrain.train_step(params, st, om, on, op, cfg_o, batch_o, 0.3, noise=noise)
  g_ref = model.flat_from_tree(g_o, device='cpu').double() * scale
  g_f32 = model.flat_from_tree(g_32, device='cpu').double() * scale
  g = s1['_grads'].cpu().double()
  tol, tol32 = TOL['360'], TOL32['360']
  for mod, b, e in model.modules:
    a, r, r32 = g[b:e], g_ref[b:e], g_f32[b:e]
    if r.norm() < 1e-12:                                              # (the proposal MLP: no loss reaches it in this configuration)
      assert a.norm() < 1e-6, mod
      continue
    cos = (a @ r / (a.norm() * r.norm() + 1e-30)).item()
    rel = ((a - r).norm() / r.norm()).item()
    rel32 = ((a - r32).norm() / r32.norm()).item()
    print(f'{mod}: grad cos {cos:.6f} rel err {rel:.3e} FP32DIST {rel32:.3e} |g| {r.norm().item():.3e}')
    assert cos > 0.995 and rel < tol['grad'], (mod, cos, rel)
    assert rel32 < tol32['grad'], (mod, rel32)


def test_two_steps_carry_the_threshold_on_the_device():
  """train.py's loop: the first step runs under 1.0 and leaves its quantile in the statistics; the second takes that device
  scalar, and its mask is the one that value implies on the second step's own rendering."""
  cfg, model, _, _, flat, batch = _setup()
  noise = helpers.make_noise(model, B_RAYS)
  state1, s1 = _step(cfg, model, flat, batch, 1.0, noise)
  thr = s1.loss_threshold_device()
  state2, s2 = _step(cfg, model, flat, batch, thr, noise, state=state1)
  assert state2.step == 2
  rgb = model._saved['levels'][-1]['rgb_out'][:B_RAYS].cpu().numpy()
  want = ref.robustnerf_mask_f64(rgb, batch.rgb.numpy(), float(thr.cpu()), **_mask_kw(cfg, B_RAYS))
  margin = np.min(np.abs(want['err'] - float(thr.cpu())) / float(thr.cpu()))
  got = model._saved['robust']['mask'][-1][:B_RAYS].cpu().numpy()
  print(f'second step: threshold {float(thr.cpu()):.6g}, closest error at a relative {margin:.3g}, mask mean {got.mean():.4f}')
  assert np.array_equal(got, want['mask'])
  assert float(model._saved['robust']['threshold'].cpu()) == float(thr.cpu())
  m1, m2 = s1.materialize(), s2.materialize()
  assert m1['loss_threshold'] == float(thr.cpu()) and m2['loss_threshold'] > 0 and 0 < m2['mask'] < 1


def test_batch_that_is_not_whole_patches_is_refused():
  cfg, model, _, _, flat, batch = _setup()
  small = helpers.synthetic_rays(300, near=cfg.near, far=cfg.far)
  with pytest.raises(ValueError, match='multiple of patch_size'):
    _step(cfg, model, flat, small, 1.0, helpers.make_noise(model, 300))
