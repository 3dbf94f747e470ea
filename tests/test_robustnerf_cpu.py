"""RobustNeRF without a GPU: the 360_robustnerf preset against what the reference's configs/360_robustnerf.gin binds, the
train step's acceptance of the loss type, the tests' float64 restatement of the mask against the reference's recorded outputs
(tests/golden/robustnerf.npz), and the new C-ABI entries in the header, the ctypes prototypes and both simulator libraries."""

import ctypes as C
import json
import os

import numpy as np
import pytest

from multinerf_amd import _lib as L
from multinerf_amd import configs, gin, models, train_utils
from tests import robustnerf_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ('mnr_robustnerf_mask', 'mnr_quantile')


def _reference_bindings():
  with open(os.path.join(HERE, 'golden', 'reference_gin_bindings_robustnerf.json')) as f:
    rec = json.load(f)['360_robustnerf']
  return {t: {a: gin._parse_value(v) for a, v in b.items()} for t, b in rec.items()}


def test_preset_binds_what_the_reference_file_binds():
  want = _reference_bindings()
  assert want['Config']['data_loss_type'] == 'robustnerf' and want['Config']['patch_size'] == 16
  gin.clear_config()
  gin.parse_config(configs.PRESETS['360_robustnerf'], skip_unknown=False)
  got = {t: dict(b) for t, b in gin._BINDINGS.items()}
  gin.clear_config()
  assert got == want
  cfg = configs.load_preset('360_robustnerf')
  assert cfg.data_loss_type == 'robustnerf' and cfg.patch_size == 16 and cfg.enable_robustnerf_loss is True
  assert cfg.robustnerf_inlier_quantile == 0.8 and cfg.robustnerf_inner_patch_size == 8
  # ... and it is 360.gin plus the four RobustNeRF bindings
  base = configs.load_preset('360')
  import dataclasses
  diff = {k for k, v in dataclasses.asdict(cfg).items() if v != getattr(base, k)}
  assert diff == {'patch_size', 'data_loss_type', 'robustnerf_inlier_quantile', 'enable_robustnerf_loss'}


def _model(cfg):
  m = models.Model(config=cfg)
  m.build('cpu')                                                      # (the parameter layout only: nothing is launched)
  return m


def test_create_train_step_accepts_the_loss_type():
  cfg = configs.load_preset('360_robustnerf', ['NerfMLP.net_width = 256', 'PropMLP.net_width = 128'])
  step = train_utils.create_train_step(_model(cfg), cfg)
  assert callable(step)
  bad = configs.load_preset('360_robustnerf', ['NerfMLP.net_width = 256', 'PropMLP.net_width = 128', 'Config.robustnerf_inner_patch_size = 32'])
  with pytest.raises(ValueError, match='robustnerf_inner_patch_size'):
    train_utils.create_train_step(_model(bad), bad)
  other = configs.load_preset('360', ['NerfMLP.net_width = 256', 'PropMLP.net_width = 128', "Config.data_loss_type = 'huber'"])
  with pytest.raises(NotImplementedError, match='out of scope'):
    train_utils.create_train_step(_model(other), other)


def test_train_stats_expose_the_robust_statistics():
  import torch
  n = 3
  raw = torch.arange(4 * n + 11, dtype=torch.float32) + 1.0
  s = train_utils.TrainStats({'_raw': raw, '_nlev': n, 'grad_sqnorms': torch.ones(2), '_robust': True, '_robust_on': True})
  m = s.materialize()
  k = 4 * n + 6
  assert [m[x] for x in ('loss_threshold', 'is_inlier_loss', 'has_inlier_neighbors', 'is_inlier_patch', 'mask')] == [float(raw[k + i]) for i in range(5)]
  t = s.loss_threshold_device()
  assert t.dim() == 0 and t.data_ptr() == raw[k:].data_ptr()          # a view: nothing is copied or read back
  plain = train_utils.TrainStats({'_raw': raw[:4 * n + 6], '_nlev': n, 'grad_sqnorms': torch.ones(2)})
  assert 'loss_threshold' not in plain.materialize()
  with pytest.raises(KeyError):
    plain.loss_threshold_device()


def test_float64_restatement_equals_the_reference():
  z = np.load(os.path.join(HERE, 'golden', 'robustnerf.npz'))
  names = sorted({k.split('/')[0] for k in z.files})
  assert len(names) == 9
  for name in names:
    g = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
    P, inner, f, B_valid, enable = (int(v) for v in g['params'])
    qs, qp, qi = (float(v) for v in g['quantiles'])
    assert g['rgb'].dtype == np.float32 and g['gt'].dtype == np.float32 and g['lossmult'].dtype == np.float32
    # (the mid thresholds are float32 values; 1e30 rounds by 1.5e-8, far inside the 1e-5 the errors keep clear of it)
    assert abs(float(np.float32(g['threshold'])) - float(g['threshold'])) <= 1e-7 * float(g['threshold'])
    out = ref.robustnerf_mask_f64(g['rgb'], g['gt'], float(g['threshold']), B_valid=B_valid, patch_size=P, inner_patch_size=inner,
                                  filter_size=f, smoothed_inlier_quantile=qs, inner_patch_inlier_quantile=qp, enable=bool(enable))
    assert np.array_equal(out['mask'], g['mask']), name
    for k, nm in enumerate(ref.STAT_NAMES):
      assert abs(out['stats'].get(nm, 0.0) - g['stats'][k]) <= 1e-12, (name, nm)
    assert abs(ref.weighted_mse(g['rgb'], g['gt'], g['lossmult'], B_valid) - float(g['mse'])) <= 1e-12 * float(g['mse'])
    assert abs(np.quantile(out['err'], qi) - float(g['next_threshold'])) <= 1e-12 * float(g['next_threshold'])
    # what the generator promised: no error within a relative 1e-5 of the threshold, no vote on a tie
    thr = float(g['threshold'])
    assert np.all(np.abs(out['err'] - thr) > 1e-5 * thr), name
    if enable:
      assert np.all(np.abs(out['box_votes'] / f ** 2 - (1 - qs)) > 1e-9) and np.all(np.abs(out['patch_votes'] / P ** 2 - (1 - qp)) > 1e-9)
    assert np.array_equal(g['lossmult_masked'], g['lossmult'].astype(np.float64) * g['mask'][:, None])


def test_inner_patch_rectangle_splits_an_odd_difference_like_the_reference():
  # robustnerf.py:104-105: lower = (outer - inner) // 2, the rest above; 8 - 3 = 5 -> rows / columns 2..4
  rgb = np.zeros((64, 3))
  out = ref.robustnerf_mask_f64(rgb + 1.0, rgb, 2.0, B_valid=64, patch_size=8, inner_patch_size=3, filter_size=3,
                                smoothed_inlier_quantile=0.5, inner_patch_inlier_quantile=0.5)
  assert out['stats']['is_inlier_patch'] == 9 / 64 and out['parts']['patch'].reshape(8, 8)[2:5, 2:5].all()


def test_header_prototypes_and_libraries_agree_on_the_new_symbols():
  from tests import sim_helpers
  header = L.header_symbols()
  for name in NEW_SYMBOLS:
    assert name in header and name in L._PROTOS, name
    assert name not in L.F32_ABSENT
  assert L._PROTOS['mnr_quantile'][0][2] is C.c_double
  for f32 in (False, True):
    lib = sim_helpers.load_sim(f32=f32)
    for name in NEW_SYMBOLS:
      assert hasattr(lib, name), (name, f32)
  # the gfx950 builds: the product library and the fp32-Dense debug library
  if not (os.path.exists(L.LIB_PATH) and os.path.exists(L.LIB_F32_PATH)):
    import __graft_entry__
    __graft_entry__.build()
  hip, hip_f32 = L.load(), C.CDLL(L.LIB_F32_PATH)
  for name in NEW_SYMBOLS:
    assert hasattr(hip, name) and hasattr(hip_f32, name), name
  assert hip.mnr_abi_version() == 21 and hip_f32.mnr_abi_version() == 21
  # the struct the header declares and the ctypes mirror have the same size on the host side of the simulator
  assert C.sizeof(L.RobustArgs) == 8 * 2 + 4 * 4 + 8 * 2 + 8 * 3 + 8 + 8 * 7
  assert sim_helpers.load_sim().mnr_abi_version() == 21
