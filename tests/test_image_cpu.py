"""CPU checks of the evaluation metrics: the float64 restatements (tests/image_ref.py) against the reference's recorded
outputs (tests/golden/image_metrics.npz) and against an independent formulation, the Gram + lstsq form of the colour
correction the device code uses, the host-side functions of multinerf_amd.image, and the config / rejection paths.  No
GPU, nothing outside the repository is read."""

import ctypes as C
import dataclasses
import math
import os
import types

import numpy as np
import pytest
import torch

from multinerf_amd import _lib as L
from multinerf_amd import configs, image, ops
from tests import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'image_metrics.npz')
CASE_NAMES = ['cast', 'grey', 'identical', 'odd', 'crop']
NEW_SYMBOLS = ['mnr_ssim', 'mnr_ssim_partials', 'mnr_image_sqdiff', 'mnr_image_sqdiff_partials', 'mnr_cc_gram',
               'mnr_cc_gram_partials', 'mnr_cc_apply']
EPS = 0.5 / 255


@pytest.fixture(scope='module')
def golden_cases():
  z = np.load(GOLDEN)                                       # (allow_pickle stays False: arrays only)
  assert os.path.getsize(GOLDEN) < (1 << 20)
  names = sorted({k.split('/')[0] for k in z.files})
  assert names == sorted(CASE_NAMES)
  return {n: {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(n + '/')} for n in names}


def _scipy_ssim(a, b, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
  """An independent formulation: scipy's 1-D correlation along each axis ('constant' padding), cut to the VALID part."""
  from scipy.ndimage import correlate1d
  h = filter_size // 2
  w = np.exp(-0.5 * ((np.arange(filter_size) - h) / filter_sigma)**2)
  w /= w.sum()
  filt = lambda z: correlate1d(correlate1d(z, w, axis=0, mode='constant'), w, axis=1, mode='constant')[h:z.shape[0] - h, h:z.shape[1] - h]
  mu0, mu1 = filt(a), filt(b)
  s00 = np.maximum(ref.F32_EPS**2, filt(a * a) - mu0 * mu0)
  s11 = np.maximum(ref.F32_EPS**2, filt(b * b) - mu1 * mu1)
  s01 = filt(a * b) - mu0 * mu1
  s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
  c1, c2 = k1**2, k2**2
  return float(np.mean((2 * mu0 * mu1 + c1) * (2 * s01 + c2) / ((mu0**2 + mu1**2 + c1) * (s00 + s11 + c2))))


@pytest.mark.parametrize('name', CASE_NAMES)
def test_ssim_restatement_equals_an_independent_formulation(golden_cases, name):
  g = golden_cases[name]
  a, b = g['img'].astype(np.float64), g['ref'].astype(np.float64)
  assert abs(ref.ssim(a, b) - _scipy_ssim(a, b)) <= 1e-13
  assert abs(ref.ssim(a, b, filter_size=5, filter_sigma=0.8) - _scipy_ssim(a, b, 5, 0.8)) <= 1e-13


def test_ssim_restatement_closed_forms():
  rs = np.random.RandomState(0)
  x = rs.uniform(0, 1, (30, 41, 3))
  assert ref.ssim(x, x) == 1.0
  ca, cb = 0.25, 0.75
  got = ref.ssim(np.full((20, 25, 1), ca), np.full((20, 25, 1), cb))
  # sigma01 = 0 and both sigmas sit at their floor eps^2: the structure term is c2 / (2 eps^2 + c2)
  want = (2 * ca * cb + 1e-4) / (ca * ca + cb * cb + 1e-4) * 9e-4 / (2 * ref.F32_EPS**2 + 9e-4)
  assert abs(got - want) <= 1e-13
  assert abs(ref.gaussian_window().sum() - 1.0) <= 1e-15 and ref.gaussian_window().argmax() == 5


@pytest.mark.parametrize('name', CASE_NAMES)
def test_restatements_equal_the_fixture(golden_cases, name):
  """The step-by-step colour correction equals the reference's (two lstsq calls on the same matrices: 1e-9 covers the
  rank-deficient case), and eval.py:134-146's preparation + MetricHarness equals the recorded metrics."""
  g = golden_cases[name]
  img, gt = g['img'].astype(np.float64), g['ref'].astype(np.float64)
  assert float(np.abs(ref.color_correct(img, gt) - g['cc']).max()) <= 1e-9
  for crop in (int(c) for c in g['crops']):
    for q in (0, 1):
      for tag, pred in (('metric', img), ('metric_cc', g['cc'])):
        with np.errstate(divide='ignore'):
          m = ref.metric_harness(pred, gt, quantize=bool(q), crop=crop)
        want = g[f'{tag}/q{q}c{crop}']
        assert (m['psnr'] == want[0] or abs(m['psnr'] - want[0]) <= 1e-9) and abs(m['ssim'] - want[1]) <= 1e-13, (tag, q, crop)
        # handing SSIM the float32 roundings of its inputs (jax, and the device code) moves it far less than a printed digit
        assert abs(ref.metric_harness(pred, gt, quantize=bool(q), crop=crop, cast_f32=True)['ssim'] - want[1]) <= 1e-6


@pytest.mark.parametrize('name', CASE_NAMES)
def test_gram_lstsq_form_equals_the_reference(golden_cases, name):
  """The device form (10 x 10 normal equations per channel, numpy.linalg.lstsq) with the sums taken in NumPy: the same
  8-bit image as the reference's lstsq on the [pixels, 10] system, and 1e-11 before quantisation (2.2e-13 measured at
  cond(G) = 1.1e4; the grey case is rank deficient, where a plain solve would fail)."""
  g = golden_cases[name]
  img, gt = g['img'].astype(np.float64), g['ref'].astype(np.float64)
  cc = ref.color_correct_gram(img, gt, image.solve_warp)
  d = float(np.abs(cc - g['cc']).max())
  print(f'{name}: Gram + lstsq form against the reference: max abs diff {d:.3g}')
  assert d <= 1e-11
  assert np.array_equal(np.round(cc * 255), np.round(g['cc'] * 255))
  if name == 'grey':
    G = np.zeros((10, 10))
    G[np.triu_indices(10)] = ref.gram_sums(img.reshape(-1, 3), gt.reshape(-1, 3), ref.unclipped(img.reshape(-1, 3), EPS), EPS)[0, :55]
    assert np.linalg.matrix_rank(G + np.triu(G, 1).T) == 3


def test_fixture_keeps_its_margins(golden_cases):
  """What tests/golden/make_golden_image.py asserts, re-checked on the committed file: no value of a corrected image
  within 1e-6 of a rounding tie, no tested value within 1e-9 of eps or 1 - eps, and in the colour-cast case each of the
  three mask terms removes rows the other two would keep."""
  for name, g in golden_cases.items():
    cc = g['cc']
    frac = cc * 255 - np.floor(cc * 255)
    assert float(np.abs(frac - 0.5).min()) / 255 > 1e-6, name
    trace = []
    ref.color_correct(g['img'].astype(np.float64), g['ref'].astype(np.float64), trace=trace)
    tested = np.concatenate([t[0].ravel() for t in trace] + [g['ref'].astype(np.float64).ravel()])
    assert min(np.abs(tested - EPS).min(), np.abs(tested - (1 - EPS)).min()) > 1e-9, name
    if name == 'cast':
      alone = np.zeros(3, np.int64)
      for _, m0, cur, refu in trace:
        alone += [(~m0 & cur & refu).sum(), (m0 & ~cur & refu).sum(), (m0 & cur & ~refu).sum()]
      assert alone.min() > 0, alone
  assert golden_cases['odd']['img'].shape == (75, 93, 3) and list(golden_cases['crop']['crops']) == [0, 6]
  assert np.array_equal(golden_cases['identical']['img'], golden_cases['identical']['ref'])
  grey = golden_cases['grey']['img']
  assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])


def test_host_side_image_functions_equal_the_reference(golden_cases):
  g = golden_cases['cast']
  x = torch.as_tensor(g['img'].astype(np.float64))
  assert float((image.linear_to_srgb(x) - torch.as_tensor(g['linear_to_srgb'])).abs().max()) <= 1e-14
  assert float((image.srgb_to_linear(x) - torch.as_tensor(g['srgb_to_linear'])).abs().max()) <= 1e-14
  assert float((image.downsample(x, 4) - torch.as_tensor(g['downsample4'])).abs().max()) <= 1e-14
  with pytest.raises(ValueError, match='does not evenly divide'):
    image.downsample(x, 7)
  assert abs(image.mse_to_psnr(0.01) - 20.0) <= 1e-12 and image.mse_to_psnr(0.0) == math.inf
  assert abs(image.psnr_to_mse(image.mse_to_psnr(0.037)) - 0.037) <= 1e-15
  assert abs(float(image.mse_to_psnr(torch.tensor(0.01, dtype=torch.float64))) - 20.0) <= 1e-12
  assert image.ssim_to_dssim(0.8) == pytest.approx(0.1) and image.dssim_to_ssim(image.ssim_to_dssim(0.8)) == pytest.approx(0.8)


def test_solve_warp_handles_full_and_deficient_rank():
  rs = np.random.RandomState(1)
  A = ref.features(rs.uniform(0.1, 0.9, (500, 3)))
  w_true = rs.standard_normal((10, 3))
  gram = np.zeros((3, 65))
  for c in range(3):
    gram[c, :55] = (A.T @ A)[np.triu_indices(10)]
    gram[c, 55:] = A.T @ (A @ w_true[:, c])
  assert float(np.abs(image.solve_warp(gram) - w_true).max()) <= 1e-6
  x = rs.uniform(0.1, 0.9, (500, 1))
  A = ref.features(np.repeat(x, 3, 1))                      # grey: rank 3
  b = 0.2 + 0.5 * x[:, 0] + 0.3 * x[:, 0]**2
  for c in range(3):
    gram[c, :55] = (A.T @ A)[np.triu_indices(10)]
    gram[c, 55:] = A.T @ b
  w = image.solve_warp(gram)
  assert np.all(np.isfinite(w)) and float(np.abs(A @ w[:, 0] - b).max()) <= 1e-10
  assert float(np.abs(w[:, 0] - np.linalg.lstsq(A, b, rcond=-1)[0]).max()) <= 1e-10       # the minimum-norm solution


def test_host_tensors_and_unsupported_settings_are_refused():
  x = torch.zeros((24, 30, 3))
  with pytest.raises(ValueError, match='no CPU fallback'):
    ops.ssim(x, x)
  with pytest.raises(ValueError, match='no CPU fallback'):
    ops.image_sqdiff(x, x)
  with pytest.raises(ValueError, match='no CPU fallback'):
    ops.cc_gram(x.reshape(-1, 3).double(), x.reshape(-1, 3).double(), torch.zeros((720, 3), dtype=torch.uint8), EPS)
  with pytest.raises(ValueError, match='no CPU fallback'):
    ops.cc_apply(x.reshape(-1, 3).double(), [[0.0] * 3] * 10)
  with pytest.raises(ValueError, match='no CPU fallback'):
    image.color_correct(x, x)
  with pytest.raises(ValueError, match='channels must match'):
    image.color_correct(x, x[..., :2])
  with pytest.raises(ValueError, match='no CPU fallback'):
    image.MetricHarness()(x, x)
  config = dataclasses.replace(configs.Config(), eval_raw_affine_cc=True)
  with pytest.raises(ValueError, match='eval_raw_affine_cc = True is not supported'):
    image.evaluate_image({'rgb': x}, types.SimpleNamespace(rgb=x), config)
  c = configs.Config()
  assert c.eval_quantize_metrics is True and c.eval_crop_borders == 0 and c.eval_render_interval == 1
  assert c.compute_disp_metrics is False and c.eval_raw_affine_cc is False


def test_header_prototypes_and_libraries_agree_on_the_new_symbols():
  from tests import sim_helpers
  header = L.header_symbols()
  for name in NEW_SYMBOLS:
    assert name in header and name in L._PROTOS, name
    assert name not in L.F32_ABSENT
  for f32 in (False, True):
    lib = sim_helpers.load_sim(f32=f32)
    for name in NEW_SYMBOLS:
      assert hasattr(lib, name), (name, f32)
  if not (os.path.exists(L.LIB_PATH) and os.path.exists(L.LIB_F32_PATH)):
    from multinerf_amd import build
    build.build(verbose=False)
  hip, hip_f32 = L.load(), C.CDLL(L.LIB_F32_PATH)
  for name in NEW_SYMBOLS:
    assert hasattr(hip, name) and hasattr(hip_f32, name), name
  assert hip.mnr_abi_version() == 21 and hip_f32.mnr_abi_version() == 21
  # the ctypes mirrors have the layout the header declares (LP64: ints packed in fours, then 8-byte members)
  assert C.sizeof(L.SsimArgs) == 4 * 5 + 4 + 8 * 4 + 8 * 5
  assert C.sizeof(L.SqdiffArgs) == 4 * 7 + 4 + 8 * 5
  assert C.sizeof(L.CcGramArgs) == 8 * 2 + 8 * 3 + 4 + 4 + 8 * 2
  assert L.SSIM_MAX_FILTER == 11 and L.CC_GRAM_OUT == 55 + L.CC_FEATURES
  # the workspace sizes the host allocates: one double per SSIM tile and channel, and the invalid shapes answer 0
  assert hip.mnr_ssim_partials(75, 93, 3, 0, 11) == 3 * 5 * 3 and hip.mnr_ssim_partials(10, 93, 3, 0, 11) == 0
  assert hip.mnr_image_sqdiff_partials(1000) == 4 and hip.mnr_cc_gram_partials(1000) == 4 * 3 * 65 and hip.mnr_cc_gram_partials(10**6) == 512 * 3 * 65


def test_metrics_source_is_in_every_source_list():
  import importlib.util
  from multinerf_amd import build
  assert 'metrics.hip' in build.SOURCES and 'metrics.hip' in build.SOURCES_F32
  for rel, attr in (('tools/hipsim/build.py', 'SOURCES'), ('tools/isa_report.py', 'KERNEL_FILES')):
    spec = importlib.util.spec_from_file_location('m_' + attr, os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'metrics.hip' in getattr(mod, attr), rel
