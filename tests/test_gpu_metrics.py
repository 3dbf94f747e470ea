"""Evaluation metrics on the GPU (-m gpu): mnr_ssim, mnr_image_sqdiff and the colour-correction entries (mnr_cc_gram,
mnr_cc_apply) against the reference's own outputs (tests/golden/image_metrics.npz, made by
tests/golden/make_golden_image.py) and the float64 restatements of tests/image_ref.py; then image.evaluate_image against
the reference-order computation in NumPy float64, and train.py / eval.py end to end.

Bounds.
  * Corrected image.  The fixture keeps every pre-quantisation value further than 1e-6 from a rounding tie, so the
    corrected image must quantise to exactly the reference's 8-bit image: zero differing values.  Before quantisation the
    difference to the fixture is the conditioning of the 10 x 10 normal equations times the float64 rounding of their
    sums; CC_BOUND is ten times the largest value measured on the MI355X over the cases, 2.93e-14 (cast 1.22e-14, grey
    2.89e-15, identical 1.73e-14, odd 2.93e-14, crop 1.42e-14; the factor covers the summation order of another
    workgroup count: an earlier version with twice the workgroups measured 1.85e-14 at worst).  The same form with the sums taken by NumPy on the host gives up to 1.5e-13.
  * SSIM.  The kernel takes float32 images and sums in float64, as the restatement does when handed the same float32
    values.  Measured on the MI355X: at most 3.3e-16 over every case, crop and quantisation (1.5 ulp of the result).
    SSIM_BOUND is a hundred times that: the NumPy side is not bit-stable either (its exp for the window and its pairwise
    mean may differ in the last place between CPUs), and 150 ulp is still nine orders below a printed digit.  Against the
    fixture (the reference's MetricHarness on float64 arrays, which jax would round to float32 first; measured up to
    9.9e-9) the bound is 5e-5 whatever was measured: the scripts print four decimals.
  * PSNR.  A float64 sum of squares in another order than NumPy's mean: 1e-9 dB.
  * Two runs agree bit for bit (no floating-point atomics).
The figures are printed before they are asserted.
"""

import dataclasses
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import configs, image, ops
from tests import image_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'image_metrics.npz')
CASE_NAMES = ['cast', 'grey', 'identical', 'odd', 'crop']
EPS = 0.5 / 255

CC_BOUND = 2.93e-13        # 10 x 2.93e-14 measured (profiles/eval_metrics.md)
SSIM_BOUND = 3.3e-14       # 100 x 3.3e-16 measured (profiles/eval_metrics.md)
SSIM_PRINT_BOUND = 5e-5
PSNR_BOUND = 1e-9


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


def _dev(x, dtype=torch.float32):
  return torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float64)), dtype=dtype).cuda()


def _combos(g):
  return [(q, int(c)) for c in g['crops'] for q in (0, 1)]


def _psnr_close(got, want):
  return got == want if math.isinf(want) else abs(got - want) <= PSNR_BOUND


# ----------------------------------------------------------------------------- kernels


@pytest.mark.parametrize('name', CASE_NAMES)
def test_ssim_kernel_equals_the_restatement(golden_cases, name):
  g = golden_cases[name]
  a, b = _dev(g['img']), _dev(g['ref'])
  a64, b64 = g['img'].astype(np.float64), g['ref'].astype(np.float64)
  for crop in (int(c) for c in g['crops']):
    out, smap = ops.ssim(a, b, crop=crop, return_map=True)
    again = ops.ssim(a, b, crop=crop)
    torch.cuda.synchronize()
    got = float(out.cpu()[0])
    cut = (lambda z: z[crop:-crop, crop:-crop]) if crop else (lambda z: z)
    want, want_map = ref.ssim(cut(a64), cut(b64), return_map=True)
    d_map = float(np.abs(smap.cpu().numpy().astype(np.float64) - want_map).max())
    print(f'{name} crop {crop}: ssim kernel {got:.15g} restatement {want:.15g} diff {abs(got - want):.3g}; map {tuple(smap.shape)} '
          f'max diff {d_map:.3g}; fixture {float(g[f"metric/q0c{crop}"][1]):.15g}')
    assert abs(got - want) <= SSIM_BOUND
    assert tuple(smap.shape) == want_map.shape and d_map <= 2.0**-22          # the map is float32, |ssim| <= 1
    assert abs(got - float(g[f'metric/q0c{crop}'][1])) <= SSIM_PRINT_BOUND
    assert out.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()         # bit for bit


def test_ssim_kernel_closed_forms():
  """ssim(x, x) = 1; two constant images a, b: (2ab + c1) / (a^2 + b^2 + c1) (sigma01 = 0, the sigmas at their floor;
  filt(a a) - mu^2 is 0 up to 11 roundings of a^2 = 1e-16, against c2 = 9e-4: 1e-12 covers it, 2.8e-14 measured); other
  window sizes against the restatement."""
  rs = np.random.RandomState(3)
  x = _dev(rs.uniform(0, 1, (37, 51, 3)))
  assert abs(float(ops.ssim(x, x).cpu()[0]) - 1.0) <= 1e-15
  ca, cb = 0.25, 0.75
  got = float(ops.ssim(torch.full((20, 45, 2), ca).cuda(), torch.full((20, 45, 2), cb).cuda()).cpu()[0])
  eps2, c1, c2 = ref.F32_EPS**2, 1e-4, 9e-4
  want = (2 * ca * cb + c1) / (ca * ca + cb * cb + c1) * c2 / (2 * eps2 + c2)
  print(f'constant images: kernel {got:.15g} closed form {want:.15g}')
  assert abs(got - want) <= 1e-12
  y = _dev(rs.uniform(0, 1, (37, 51, 3)))
  for fs, sigma, mv in ((1, 1.5, 1.0), (5, 0.8, 1.0), (7, 2.0, 2.0)):
    got = float(ops.ssim(x, y, filter_size=fs, filter_sigma=sigma, max_val=mv).cpu()[0])
    want = ref.ssim(x.cpu().numpy(), y.cpu().numpy(), filter_size=fs, filter_sigma=sigma, max_val=mv)
    print(f'filter {fs} sigma {sigma} max_val {mv}: kernel {got:.15g} restatement {want:.15g}')
    assert abs(got - want) <= SSIM_BOUND


@pytest.mark.parametrize('name', CASE_NAMES)
def test_image_sqdiff_kernel_equals_numpy(golden_cases, name):
  g = golden_cases[name]
  a64, b64, cc = g['img'].astype(np.float64), g['ref'].astype(np.float64), g['cc']
  for pred, dt in ((a64, torch.float32), (a64, torch.float64), (cc, torch.float64)):
    for q, crop in _combos(g):
      for bdt in (torch.float32, torch.float64):
        q_out = torch.full(pred.shape, -1.0).cuda()
        out = ops.image_sqdiff(_dev(pred, dt), _dev(b64, bdt), quantize=bool(q), crop=crop, q_out=q_out)
        torch.cuda.synchronize()
        pq = np.round(pred * 255) / 255 if q else pred
        cut = (lambda z: z[crop:-crop, crop:-crop]) if crop else (lambda z: z)
        want = float(((cut(pq) - cut(b64))**2).sum())
        got = float(out.cpu()[0])
        assert abs(got - want) <= 1e-12 * max(want, 1e-30), (name, q, crop, got, want)
        assert np.array_equal(q_out.cpu().numpy(), pq.astype(np.float32))       # the whole image, crop or not
  print(f'{name}: sums of squares match NumPy to 1e-12 relative over {len(_combos(g)) * 6} variants')


@pytest.mark.parametrize('name', CASE_NAMES)
def test_cc_gram_and_apply_kernels_equal_numpy(golden_cases, name):
  """One iteration's sums against NumPy on the same rows (1e-12 relative to the largest entry: float64 sums of at most
  ~2e4 terms in [0, 1] in another order), the mask that iteration writes, bit equality of two runs, and the apply."""
  g = golden_cases[name]
  img, gt = g['img'].astype(np.float64).reshape(-1, 3), g['ref'].astype(np.float64).reshape(-1, 3)
  d_img, d_ref = _dev(img, torch.float64), _dev(gt, torch.float64)
  mask0 = torch.full(img.shape, 7, dtype=torch.uint8).cuda()
  gram = ops.cc_gram(d_img, d_ref, mask0, EPS, write_mask0=True)
  again = ops.cc_gram(d_img, d_ref, mask0, EPS, write_mask0=False)                # (reads the mask the first call wrote)
  torch.cuda.synchronize()
  m0 = ref.unclipped(img, EPS)
  assert np.array_equal(mask0.cpu().numpy(), m0.astype(np.uint8))
  want = ref.gram_sums(img, gt, m0, EPS)
  got = gram.cpu().numpy()
  d = float(np.abs(got - want).max() / np.abs(want).max())
  print(f'{name}: {img.shape[0]} pixels, rows kept per channel {[int(v) for v in got[:, 54]]}, gram max rel diff {d:.3g}')
  assert d <= 1e-12
  assert got.tobytes() == again.cpu().numpy().tobytes()
  warp = image.solve_warp(got)
  out = ops.cc_apply(d_img, warp)
  want_img = np.clip(ref.features(img) @ warp, 0, 1)
  assert float(np.abs(out.cpu().numpy() - want_img).max()) <= 1e-14
  assert out.data_ptr() != d_img.data_ptr() and np.array_equal(d_img.cpu().numpy(), img)
  ops.cc_apply(d_img, warp, out=d_img)                                           # in place
  assert np.array_equal(d_img.cpu().numpy(), out.cpu().numpy())


@pytest.mark.parametrize('name', CASE_NAMES)
def test_color_correct_equals_the_reference(golden_cases, name):
  g = golden_cases[name]
  a, b = _dev(g['img']), _dev(g['ref'])
  cc = image.color_correct(a, b)
  cc2 = image.color_correct(a, b)
  torch.cuda.synchronize()
  assert cc.dtype == torch.float64 and cc.shape == a.shape
  got = cc.cpu().numpy()
  d = float(np.abs(got - g['cc']).max())
  n_diff = int((np.round(got * 255) != np.round(g['cc'] * 255)).sum())
  print(f'{name}: corrected image max abs diff to the reference {d:.3g}, differing 8-bit values {n_diff} of {got.size}')
  assert n_diff == 0
  assert d <= CC_BOUND
  assert got.tobytes() == cc2.cpu().numpy().tobytes()
  assert np.array_equal(a.cpu().numpy(), g['img'].astype(np.float32))            # the input is left alone


@pytest.mark.parametrize('name', CASE_NAMES)
def test_metric_harness_equals_the_reference(golden_cases, name):
  g = golden_cases[name]
  harness = image.MetricHarness()
  gt = _dev(g['ref'], torch.float64)
  for tag, pred in (('metric', g['img'].astype(np.float64)), ('metric_cc', g['cc'])):
    for q, crop in _combos(g):
      m = harness(_dev(pred, torch.float64), gt, quantize=bool(q), crop=crop)
      want_psnr, want_ssim = (float(v) for v in g[f'{tag}/q{q}c{crop}'])
      own = ref.metric_harness(pred, g['ref'], quantize=bool(q), crop=crop, cast_f32=True)
      print(f'{name} {tag} quantize {q} crop {crop}: psnr {m["psnr"]:.12g} reference {want_psnr:.12g}; ssim {m["ssim"]:.12g} '
            f'reference {want_ssim:.12g} (diff {abs(m["ssim"] - want_ssim):.3g}), restatement on float32 {own["ssim"]:.12g} '
            f'(diff {abs(m["ssim"] - own["ssim"]):.3g})')
      assert set(m) == {'psnr', 'ssim'}
      assert _psnr_close(m['psnr'], want_psnr)
      assert abs(m['ssim'] - want_ssim) <= SSIM_PRINT_BOUND
      assert abs(m['ssim'] - own['ssim']) <= SSIM_BOUND
      assert f'{m["ssim"]:.4f}' == f'{want_ssim:.4f}'                           # what the scripts print
  assert harness(gt, gt, name_fn=lambda s: 'x_' + s) == {'x_psnr': math.inf, 'x_ssim': 1.0}
  # float32 images, not quantised: SSIM reads the prediction as given (no float32 copy is made); the same numbers
  for crop in (int(c) for c in g['crops']):
    assert harness(_dev(g['img']), _dev(g['ref']), crop=crop) == harness(_dev(g['img'], torch.float64), gt, crop=crop)


def test_metrics_argument_errors_are_raised_not_launched():
  x = torch.zeros((24, 30, 3)).cuda()
  with pytest.raises(ValueError, match='smaller than the 11 x 11 window'):
    ops.ssim(x[:10].contiguous(), x[:10].contiguous())
  with pytest.raises(ValueError, match='cropped by 7 is smaller than the 11 x 11 window'):
    ops.ssim(x, x, crop=7)
  with pytest.raises(ValueError, match='filter_size 4 must be odd'):
    ops.ssim(x, x, filter_size=4)
  with pytest.raises(ValueError, match='filter_size 13 exceeds the compiled limit of 11'):
    ops.ssim(x, x, filter_size=13)
  tall = torch.zeros((16 * 65535 + 11, 11, 1)).cuda()
  with pytest.raises(ValueError, match='exceeds the limit of 1048560'):
    ops.ssim(tall, tall)
  with pytest.raises(ValueError, match='filter_sigma'):
    ops.ssim(x, x, filter_sigma=0.0)
  with pytest.raises(ValueError, match='one shape'):
    ops.ssim(x, x[:, :20].contiguous())
  with pytest.raises(ValueError, match='float32'):
    ops.ssim(x.double(), x.double())
  with pytest.raises(ValueError, match='cropped by 12 is empty'):
    ops.image_sqdiff(x, x, crop=12)
  d = torch.zeros((50, 3), dtype=torch.float64).cuda()
  m = torch.zeros((50, 3), dtype=torch.uint8).cuda()
  with pytest.raises(ValueError, match=r'eps = 0.7 is outside \[0, 0.5\)'):
    ops.cc_gram(d, d, m, 0.7)
  with pytest.raises(ValueError, match=r'must be \[N,3\]'):
    ops.cc_gram(d, d[:40].contiguous(), m, EPS)
  with pytest.raises(ValueError, match='float64'):
    ops.cc_gram(d.float(), d, m, EPS)
  with pytest.raises(ValueError, match='not finite'):
    ops.cc_apply(d, [[float('nan')] * 3] * 10)
  with pytest.raises(ValueError, match=r'warp must be \[10,3\]'):
    ops.cc_apply(d, [[0.0] * 3] * 9)
  with pytest.raises(ValueError, match='channels must match'):
    image.color_correct(x, x[..., :2].contiguous())


# ----------------------------------------------------------------------------- composed


def _weighted_mae(weights, n, ngt):
  """ref_utils.py:40-50 in float64."""
  l2n = lambda v: v / np.sqrt(np.maximum((v * v).sum(-1, keepdims=True), ref.F32_EPS))
  dot = (l2n(n) * l2n(ngt)).sum(-1)
  one_eps = 1 - ref.F32_EPS
  return float((weights * np.arccos(np.clip(dot, -one_eps, one_eps))).sum() / weights.sum() * 180 / np.pi)


@pytest.mark.parametrize('quant,crop', [(True, 6), (False, 0)])
def test_evaluate_image_equals_the_reference_order_computation(golden_cases, quant, crop):
  """image.evaluate_image on a synthetic rendering / batch against eval.py:118-163 restated in NumPy float64: colour
  correction, quantisation, crop, MetricHarness on both versions, disparity mse and the normal MAEs with hand-made disps,
  normals and alphas.  PSNR / SSIM bounds as above; the disparity and normal metrics come from the float32 one-workgroup
  kernel train_utils uses (mnr_render_metrics): N * 2^-23 relative for its float32 sums over N = 3072 pixels."""
  g = golden_cases['crop']
  H, W = g['img'].shape[:2]
  rs = np.random.RandomState(11)
  f32 = lambda z: z.astype(np.float32)
  dist_mean, dist_med = f32(rs.uniform(2, 6, (H, W))), f32(rs.uniform(2, 6, (H, W)))
  disps = f32(1 / (1 + dist_mean) + 0.01 * rs.standard_normal((H, W)))
  acc, alphas = f32(rs.uniform(0, 1, (H, W))), f32((rs.uniform(size=(H, W)) < 0.7).astype(np.float64))
  ngt = f32(rs.standard_normal((H, W, 3)))
  normals, normals_pred = f32(ngt + 0.3 * rs.standard_normal((H, W, 3))), f32(ngt + 0.6 * rs.standard_normal((H, W, 3)))
  rendering = {'rgb': _dev(g['img']), 'distance_mean': _dev(dist_mean), 'distance_median': _dev(dist_med), 'acc': _dev(acc),
               'normals': _dev(normals), 'normals_pred': _dev(normals_pred), 'roughness': None}
  batch = types.SimpleNamespace(rgb=_dev(g['ref']), disps=_dev(disps), normals=_dev(ngt), alphas=_dev(alphas))
  config = dataclasses.replace(configs.Config(), eval_quantize_metrics=quant, eval_crop_borders=crop, compute_disp_metrics=True,
                               compute_normal_metrics=True)
  metric, metric_cc, images = image.evaluate_image(rendering, batch, config, image.MetricHarness())
  img64, gt64 = g['img'].astype(np.float64), g['ref'].astype(np.float64)
  cc = ref.color_correct(img64, gt64)
  want = ref.metric_harness(img64, gt64, quantize=quant, crop=crop, cast_f32=True)
  want_cc = ref.metric_harness(cc, gt64, quantize=quant, crop=crop, cast_f32=True)
  want['disparity_mean_mse'] = float(((1 / (1 + dist_mean.astype(np.float64)) - disps)**2).mean())
  want['disparity_median_mse'] = float(((1 / (1 + dist_med.astype(np.float64)) - disps)**2).mean())
  w = acc.astype(np.float64) * alphas
  want['normals_mae'] = _weighted_mae(w, normals.astype(np.float64), ngt.astype(np.float64))
  want['normals_pred_mae'] = _weighted_mae(w, normals_pred.astype(np.float64), ngt.astype(np.float64))
  for k in want:
    print(f'quantize {quant} crop {crop}: {k} {metric[k]:.12g} reference order {want[k]:.12g}')
  for k in want_cc:
    print(f'quantize {quant} crop {crop}: cc {k} {metric_cc[k]:.12g} reference order {want_cc[k]:.12g}')
  assert list(metric) == ['psnr', 'ssim', 'disparity_mean_mse', 'disparity_median_mse', 'normals_mae', 'normals_pred_mae']
  assert list(metric_cc) == ['psnr', 'ssim']
  for m, wnt in ((metric, want), (metric_cc, want_cc)):
    assert abs(m['psnr'] - wnt['psnr']) <= PSNR_BOUND
    assert abs(m['ssim'] - wnt['ssim']) <= SSIM_BOUND
  for k in ('disparity_mean_mse', 'disparity_median_mse', 'normals_mae', 'normals_pred_mae'):
    assert abs(metric[k] - want[k]) <= H * W * 2.0**-23 * abs(want[k]), k
  assert set(images) == {'color', 'color_cc', 'distance_mean', 'distance_median', 'normals', 'acc'}
  assert images['color_cc'] is rendering['rgb_cc'] and float(np.abs(images['color_cc'].cpu().numpy() - g['cc']).max()) <= CC_BOUND
  assert np.array_equal(image.quantize_u8(images['color_cc']), np.round(g['cc'] * 255).astype(np.uint8))
  with pytest.raises(ValueError, match='eval_raw_affine_cc'):
    image.evaluate_image(rendering, batch, dataclasses.replace(config, eval_raw_affine_cc=True))
  with pytest.raises(ValueError, match='needs batch.disps'):
    image.evaluate_image(rendering, types.SimpleNamespace(rgb=batch.rgb), config)


def test_train_then_eval_writes_metrics_the_saved_images_reproduce(tmp_path):
  """train.py then eval.py on the procedural scene in subprocesses: test_ssim is logged; eval.py writes the reference's
  files; every metric_psnr / metric_ssim value (and the colour-corrected pair) is reproduced, in NumPy float64, from the
  saved PNG and the dataset's ground truth: what Config.eval_quantize_metrics promises."""
  from PIL import Image
  from multinerf_amd import datasets
  ck = str(tmp_path / 'ckpt')
  binds = ["Config.dataset_loader = 'procedural'", f"Config.checkpoint_dir = '{ck}'", 'Config.max_steps = 40',
           'Config.batch_size = 2048', 'Config.print_every = 20', 'Config.train_render_every = 40',
           'Config.checkpoint_every = 40', 'Config.lr_delay_steps = 0', 'Config.cast_rays_in_train_step = True',
           'NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'NerfMLP.bottleneck_width = 128',
           'Config.eval_dataset_limit = 3', 'Config.render_chunk_size = 4096', 'Config.eval_render_interval = 2',
           'Config.eval_crop_borders = 4']
  args = ['--preset', 'blender_256']
  for b in binds:
    args += ['--gin_bindings', b]
  env = dict(os.environ, PYTHONPATH=ROOT)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')] + args, capture_output=True, text=True, env=env,
                     timeout=600, cwd=ROOT)
  print(r.stdout[-1500:], r.stderr[-1500:])
  assert r.returncode == 0
  log = [json.loads(l) for l in open(os.path.join(ck, 'train_log.jsonl'))]
  renders = [e for e in log if 'test_psnr' in e]
  assert renders and all(0.0 < e['test_ssim'] <= 1.0 for e in renders)
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'eval.py')] + args, capture_output=True, text=True, env=env,
                     timeout=600, cwd=ROOT)
  print(r.stdout[-3000:], r.stderr[-1500:])
  assert r.returncode == 0 and 'Average test psnr over 3 images' in r.stdout
  out = os.path.join(ck, 'test_preds')
  files = set(os.listdir(out))
  want_files = {f'metric_{n}_40.txt' for n in ('psnr', 'ssim', 'cc_psnr', 'cc_ssim')} | {'render_times_40.txt'} | \
      {f'color_{i:03d}.png' for i in range(3)} | {f'{k}_{i:03d}.{e}' for i in (0, 2) for k, e in
                                                  (('color_cc', 'png'), ('distance_mean', 'tiff'), ('distance_median', 'tiff'), ('acc', 'tiff'))}
  assert want_files <= files, sorted(want_files - files)
  assert 'color_cc_001.png' not in files                                        # eval_render_interval
  read = lambda name: [float(v) for v in open(os.path.join(out, name)).read().split()]
  assert len(read('render_times_40.txt')) == 3
  acc = np.asarray(Image.open(os.path.join(out, 'acc_000.tiff')))
  assert acc.dtype == np.float32 and acc.shape == (96, 96)
  config = configs.load_preset('blender_256', binds)
  gt = datasets.load_dataset('test', None, config, device='cuda').images.cpu().numpy().astype(np.float64)
  for tag, stem, idxs in (('metric', 'color', (0, 1, 2)), ('metric_cc', 'color_cc', (0, 2))):
    psnrs, ssims = read(f'{tag}_psnr_40.txt'), read(f'{tag}_ssim_40.txt')
    assert len(psnrs) == 3 and len(ssims) == 3
    for i in idxs:
      png = np.asarray(Image.open(os.path.join(out, f'{stem}_{i:03d}.png')), np.float64) / 255
      own = ref.metric_harness(png, gt[i], quantize=True, crop=4, cast_f32=True)
      print(f'{stem}_{i:03d}.png: psnr file {psnrs[i]:.10g} from the PNG {own["psnr"]:.10g}; ssim file {ssims[i]:.10g} from the PNG '
            f'{own["ssim"]:.10g}')
      assert abs(psnrs[i] - own['psnr']) <= PSNR_BOUND
      assert abs(ssims[i] - own['ssim']) <= SSIM_BOUND
      assert f'{"cc_" * (tag == "metric_cc")}ssim'.ljust(30) + f' = {ssims[i]:.4f}' in r.stdout
