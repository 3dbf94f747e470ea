"""The RawNeRF data path on the GPU (-m gpu): csrc/raw.hip through multinerf_amd.ops and multinerf_amd.raw_utils against
the reference's own outputs (tests/golden/raw_utils.npz, made by tests/golden/make_golden_raw.py from internal/raw_utils.py)
and the float64 restatements of tests/raw_ref.py; then the datasets' raw mode and image.evaluate_image with a
postprocess_fn.

Bounds.
  * Demosaic.  Bit-equal: the kernel evaluates the reference's float32 expression in closed form, every product is by a
    power of two, the normalisation is IEEE float64 rounded once.  The fused downsample is bit-equal to float32(mean in
    float64) of the full-resolution result.  Against the reference's recorded downsampled images, whose mean of n x n
    values was taken in float32 (n^2 - 1 additions and a division, each rounding at 2^-24 of a partial sum no larger than
    n^2 times the largest block value in magnitude), the bound is n^2 2^-24 n^2 max|v| / n^2 = n^2 2^-24 max|v|.
  * Post-processing, in float64 against the recorded float64 output: POST_BOUND is ten times the largest deviation
    measured on the MI355X over the cases (profiles/rawnerf_data.md): the device pow and the order of the three products
    of the colour matrix differ from NumPy's in the last places.  The fixture keeps every value away from the sRGB branch
    point and every srgb * 255 away from an integer, so the 8-bit output must equal the truncated recorded one exactly.
  * Percentile: 4 float64 ulps of the value (the two order statistics are exact, the interpolation has two roundings).
  * Affine match: AFFINE_BOUND is ten times the largest deviation measured on the MI355X (profiles/rawnerf_data.md); the
    slope divides two differences of means, which amplifies the order of the float64 sums.
  * Two runs agree bit for bit.
The figures are printed before they are asserted.
"""

import dataclasses
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import configs, datasets, image, ops, raw_utils
from tests import image_ref
from tests import raw_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'raw_utils.npz')
SIMULATED = os.environ.get('MNR_TESTS_ON_SIMULATOR') == '1'
DEMOSAIC_SIZES = ((2, 2), (2, 6), (4, 2), (6, 10), (34, 66))

POST_BOUND = 10 * 1.43e-15        # 10 x measured (profiles/rawnerf_data.md)
AFFINE_BOUND = 10 * 7.53e-14      # 10 x measured (profiles/rawnerf_data.md)
PSNR_BOUND = 1e-9                 # dB: float64 sums in another order than NumPy's mean
SSIM_BOUND = 1e-9                 # one float32 rounding of a float64 value that differs in its last place moves one pixel by 6e-8


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')


@pytest.fixture(scope='module')
def g():
  return np.load(GOLDEN)


def _dev(x):
  return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(t):
  return t.cpu().numpy()


# ----------------------------------------------------------------------------- mnr_raw_demosaic


@pytest.mark.parametrize('h,w', DEMOSAIC_SIZES)
def test_demosaic_kernel_is_bit_equal_to_the_reference(g, h, w):
  mosaic, want = g[f'demosaic/{h}x{w}/mosaic'], g[f'demosaic/{h}x{w}/rgb']
  from_u16 = _np(ops.raw_demosaic(_dev(mosaic)))
  from_f32 = _np(raw_utils.bilinear_demosaic(_dev(mosaic.astype(np.float32))))
  assert from_u16.dtype == np.float32 and from_u16.shape == (h, w, 3)
  assert np.array_equal(from_u16, want) and np.array_equal(from_f32, want)
  assert np.array_equal(_np(ops.raw_demosaic(_dev(mosaic))), from_u16)                      # two runs


def test_demosaic_kernel_normalises_a_stack_per_image(g):
  """N = 3 with three black / white pairs and scale != 1: (raw - black) / (white - black) * scale in float64, rounded once,
  then the reference's recorded demosaic of a float32 mosaic is reproduced by demosaicking the normalised values."""
  mosaics = np.stack([np.roll(g['demosaic/6x10/mosaic'], k, 1) for k in range(3)])
  black, white, scale = np.array([64., 60.5, 70.]), np.array([1023., 1000., 4095.]), 0.37
  got = _np(ops.raw_demosaic(_dev(mosaics), _dev(black), _dev(white), scale))
  norm = ((mosaics.astype(np.float32) - black.reshape(-1, 1, 1)) / (white - black).reshape(-1, 1, 1) * scale).astype(np.float32)
  want = _np(ops.raw_demosaic(_dev(norm)))                                                  # float32 input, no normalisation
  assert got.shape == (3, 6, 10, 3) and np.array_equal(got, want)
  # the measured values survive the demosaic: channel of the Bayer site
  ys, xs = np.meshgrid(np.arange(6), np.arange(10), indexing='ij')
  site = np.take_along_axis(got, np.broadcast_to(((ys % 2) + (xs % 2))[None, ..., None], (3, 6, 10, 1)), -1)[..., 0]
  assert np.array_equal(site, norm)


@pytest.mark.parametrize('h,w', [(8, 12), (32, 64), (24, 40)])
def test_demosaic_kernel_fused_downsample(g, h, w):
  rs = np.random.default_rng([3, h, w])
  mosaic = rs.integers(0, 1024, (2, h, w)).astype(np.uint16)
  black, white = _dev(np.array([64., 63.])), _dev(np.array([1023., 1000.]))
  full = _np(ops.raw_demosaic(_dev(mosaic), black, white, 1.25))
  for n in (2, 4, 8):
    if h % n or w % n:                                         # (8 does not divide 12: refused, as image.downsample refuses it)
      with pytest.raises(ValueError, match='must divide'):
        ops.raw_demosaic(_dev(mosaic), black, white, 1.25, n)
      continue
    got = _np(ops.raw_demosaic(_dev(mosaic), black, white, 1.25, n))
    want = np.stack([ref.block_mean(full[i], n) for i in range(2)])
    assert got.shape == (2, h // n, w // n, 3) and np.array_equal(got, want), n
    assert np.array_equal(_np(ops.raw_demosaic(_dev(mosaic), black, white, 1.25, n)), got)


# ----------------------------------------------------------------------------- mnr_raw_postprocess


@pytest.mark.parametrize('tag', ['5x7', '75x93'])
def test_postprocess_kernel_equals_the_reference(g, tag):
  raw, cam2rgb, exposure = g[f'post/{tag}/raw'], g['post/cam2rgb'], float(g[f'post/{tag}/exposure'])
  want, want_auto = g[f'post/{tag}/srgb'], g[f'post/{tag}/srgb_auto']
  worst = 0.0
  for inp in (_dev(raw), _dev(raw.astype(np.float64))):
    host = ops.raw_postprocess(inp, cam2rgb.reshape(-1), exposure)
    devx = ops.raw_postprocess(inp, cam2rgb.reshape(-1), _dev(np.array([exposure])))
    assert torch.equal(host, devx) and host.dtype == torch.float64
    f64, f32, u8 = ops.raw_postprocess(inp, cam2rgb.reshape(-1), exposure, want=('f64', 'f32', 'u8'))
    assert torch.equal(f64, host) and np.array_equal(_np(f32), _np(f64).astype(np.float32))
    assert np.array_equal(_np(u8), ref.to_u8(want))
    worst = max(worst, float(np.abs(_np(host) - want).max()))
    auto = raw_utils.postprocess_raw(inp, cam2rgb, None, want='f64')
    worst = max(worst, float(np.abs(_np(auto) - want_auto).max()))
    assert np.array_equal(_np(raw_utils.postprocess_raw(inp, cam2rgb, None, want='u8')), ref.to_u8(want_auto))
    lin = ops.raw_postprocess(inp, cam2rgb.reshape(-1), linear_only=True)
    worst_lin = float(np.abs(_np(lin) - g[f'post/{tag}/linear']).max())
    print(f'postprocess {tag} {inp.dtype}: linear max |diff| {worst_lin:.3g}')
    assert worst_lin <= POST_BOUND
  print(f'postprocess {tag}: max |diff| to the reference {worst:.3g} (bound {POST_BOUND:.3g})')
  assert worst <= POST_BOUND
  assert raw_utils.postprocess_raw(_dev(raw), cam2rgb, exposure).dtype == torch.float32
  assert np.abs(ref.postprocess(raw, cam2rgb, exposure) - want).max() <= POST_BOUND          # the restatement, for evaluate_image below


# ----------------------------------------------------------------------------- mnr_quantile_f64


def _quantile_case(n, seed):
  rs = np.random.default_rng([seed, n])
  x = rs.normal(size=n) * 10.0**rs.integers(-3, 4, n)
  if n >= 3:
    x[rs.integers(0, n, n // 3)] = np.round(x[rs.integers(0, n, n // 3)], 1)                # duplicates
    x[1] = -x[0]
  if n >= 257:
    x[rs.integers(0, n, 5)] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
  return x


def _check_quantile(x):
  xd = _dev(x)
  finite = x[np.isfinite(x)]
  for p in (0, 50, 80, 90, 97, 99, 100):
    got = float(_np(ops.quantile_f64(xd, p))[0])
    want = float(np.percentile(finite, p))
    ulps = abs(got - want) / np.spacing(abs(want)) if want != 0 else abs(got) / np.spacing(0.)
    print(f'quantile N={x.size} p={p}: {got!r} numpy {want!r} ({ulps:.1f} ulp)')
    assert ulps <= 4, (x.size, p, got, want)
  assert torch.equal(ops.quantile_f64(xd, 97), ops.quantile_f64(xd, 97))


@pytest.mark.parametrize('n', [1, 2, 3, 257])
def test_quantile_f64_kernel_equals_numpy(n):
  _check_quantile(_quantile_case(n, 5))


def test_quantile_f64_kernel_large():
  _check_quantile(_quantile_case(100003, 6))                  # several workgroups, a grid-stride loop with a ragged end


def test_quantile_f64_kernel_without_finite_values_gives_nan():
  assert np.isnan(_np(ops.quantile_f64(_dev(np.array([np.nan, np.inf, -np.inf])), 50))[0])


# ----------------------------------------------------------------------------- mnr_affine_sums / mnr_affine_apply


@pytest.mark.parametrize('tag', ['3x4', '75x93'])
def test_affine_kernels_equal_the_reference(g, tag):
  est, gt, want = g[f'affine/{tag}/est'], g[f'affine/{tag}/gt'], g[f'affine/{tag}/matched']
  got = raw_utils.match_images_affine(_dev(est), _dev(gt))
  a, b = raw_utils.best_fit_affine(_dev(gt.astype(np.float64)), _dev(est.astype(np.float64)), axis=(0, 1))
  worst = float(np.abs(_np(got) - want).max())
  worst_ab = max(float(np.abs(a - g[f'affine/{tag}/a']).max()), float(np.abs(b - g[f'affine/{tag}/b']).max()))
  print(f'affine {tag}: matched max |diff| {worst:.3g}, a / b max |diff| {worst_ab:.3g} (bound {AFFINE_BOUND:.3g})')
  assert got.dtype == torch.float64 and worst <= AFFINE_BOUND and worst_ab <= AFFINE_BOUND
  e64, g64 = _dev(est.astype(np.float64)), _dev(gt.astype(np.float64))
  s1, s2 = ops.affine_sums(e64, g64), ops.affine_sums(e64, g64)
  assert torch.equal(s1, s2)
  want_sums = np.stack([gt.astype(np.float64).sum((0, 1)), est.astype(np.float64).sum((0, 1)),
                        (gt.astype(np.float64) * est).sum((0, 1)), (gt.astype(np.float64)**2).sum((0, 1))])
  assert np.abs(_np(s1) - want_sums).max() <= 1e-12 * np.abs(want_sums).max()
  # an exact affine map of gt is undone
  a0, b0 = np.array([1.5, 0.75, 2.0]), np.array([0.125, -0.25, 0.5])
  back = raw_utils.match_images_affine(_dev(gt.astype(np.float64) * a0 + b0), _dev(gt))
  print(f'affine {tag}: round trip max |diff| {float(np.abs(_np(back) - gt).max()):.3g}')
  assert np.abs(_np(back) - gt).max() <= AFFINE_BOUND


def test_pixels_to_bayer_mask_equals_the_reference(g):
  got = raw_utils.pixels_to_bayer_mask(_dev(g['bayer/pix_x']), _dev(g['bayer/pix_y']))
  assert got.dtype == torch.float32 and np.array_equal(_np(got), g['bayer/mask'])


# ----------------------------------------------------------------------------- argument errors


def test_raw_argument_errors_are_raised_not_launched():
  m = _dev(np.zeros((4, 6), np.uint16))
  with pytest.raises(ValueError, match='even height and width'):
    ops.raw_demosaic(_dev(np.zeros((3, 6), np.uint16)))
  with pytest.raises(ValueError, match='must divide'):
    ops.raw_demosaic(m, n_downsample=4)
  with pytest.raises(ValueError, match='uint16 or float32'):
    ops.raw_demosaic(_dev(np.zeros((4, 6), np.int32)))
  with pytest.raises(ValueError, match='go together'):
    ops.raw_demosaic(m, black=_dev(np.zeros(1)))
  with pytest.raises(ValueError, match='one level per image'):
    ops.raw_demosaic(m, _dev(np.zeros(2)), _dev(np.ones(2)))
  with pytest.raises(ValueError, match='must be torch.float64'):
    ops.raw_demosaic(m, _dev(np.zeros(1, np.float32)), _dev(np.ones(1, np.float32)))
  odd = _dev(np.zeros(4 * 6 * 3 + 1, np.float32))[1:]         # contiguous, right size, starts 4 bytes past an 8-byte boundary
  with pytest.raises(ValueError, match='multiple of 8 bytes'):
    ops.raw_demosaic(m, out=odd)
  x = _dev(np.zeros((5, 3)))
  with pytest.raises(ValueError, match='expected 3'):
    ops.raw_postprocess(_dev(np.zeros((5, 4))), np.eye(3).reshape(-1), 1.)
  with pytest.raises(ValueError, match='float32 or float64'):
    ops.raw_postprocess(_dev(np.zeros((5, 3), np.int32)), np.eye(3).reshape(-1), 1.)
  with pytest.raises(ValueError, match='needs an exposure'):
    ops.raw_postprocess(x, np.eye(3).reshape(-1))
  with pytest.raises(ValueError, match=r'expected \(3, 3\)'):
    raw_utils.postprocess_raw(x, np.eye(4), 1.)
  with pytest.raises(ValueError, match='must name some of'):
    ops.raw_postprocess(x, np.eye(3).reshape(-1), 1., want=('f16',))
  with pytest.raises(ValueError, match='must be torch.float64'):
    ops.quantile_f64(_dev(np.zeros(4, np.float32)), 50)
  with pytest.raises(ValueError, match=r'outside \[0, 100\]'):
    ops.quantile_f64(_dev(np.zeros(4)), 101)
  with pytest.raises(ValueError, match='one shape'):
    ops.affine_sums(x, _dev(np.zeros((6, 3))))
  with pytest.raises(ValueError, match='must be torch.float64'):
    ops.affine_sums(_dev(np.zeros((5, 3), np.float32)), _dev(np.zeros((5, 3), np.float32)))
  with pytest.raises(ValueError, match='three values'):
    ops.affine_apply(x, [1., 1.], [0., 0., 0.])
  if not SIMULATED:                                            # (the simulator takes host tensors by design)
    host = torch.zeros((4, 6), dtype=torch.float32)
    with pytest.raises(ValueError, match='device tensor'):
      ops.raw_demosaic(host)
    with pytest.raises(ValueError, match='device tensor'):
      ops.raw_postprocess(torch.zeros((5, 3)), np.eye(3).reshape(-1), 1.)
    with pytest.raises(ValueError, match='device tensor'):
      ops.quantile_f64(torch.zeros(4, dtype=torch.float64), 50)
    with pytest.raises(ValueError, match='device tensor'):
      raw_utils.match_images_affine(torch.zeros((2, 2, 3)), torch.zeros((2, 2, 3)))


# ----------------------------------------------------------------------------- datasets


def _check_dataset_against_golden(g, tag, images, meta, n_down=1, full=None):
  want = g[f'{tag}/images']
  got = _np(images)
  assert got.shape == want.shape and got.dtype == np.float32
  if n_down == 1:
    assert np.array_equal(got, want), tag
  else:                                                       # (module docstring: the recorded mean was taken in float32)
    assert np.array_equal(got, np.stack([ref.block_mean(im, n_down) for im in full]))
    bound = n_down**2 * 2.0**-24 * np.abs(full).max()
    print(f'{tag}: downsampled images differ from the recorded float32 mean by {np.abs(got - want).max():.3g} (bound {bound:.3g})')
    assert np.abs(got.astype(np.float64) - want).max() <= bound
  for k in ('exposure_idx', 'exposure_values', 'unique_shutters', 'cam2rgb'):
    assert np.array_equal(np.asarray(meta[k]), g[f'{tag}/{k}']), (tag, k)
  lev = np.array([meta['exposure_levels'][p] for p in (80, 90, 97, 99, 100)])
  for got_v, want_v in zip([meta['exposure']] + list(lev), [float(g[f'{tag}/exposure'])] + list(g[f'{tag}/exposure_levels'])):
    assert abs(got_v - want_v) <= 4 * np.spacing(abs(want_v)) + POST_BOUND, (tag, got_v, want_v)


def _raw_config(extra=()):
  return configs.load_preset('llff_raw', ['Config.batch_size = 64', 'Config.factor = 0'] + list(extra))


def test_llff_raw_plain_scene_dataset(g, tmp_path):
  rs = np.random.default_rng(1)
  names = ref.write_plain_scene(g, str(tmp_path), rs)
  images, meta, testscene = raw_utils.load_raw_dataset('train', str(tmp_path), names, 97., 1, 'cuda')
  assert not testscene
  _check_dataset_against_golden(g, 'plain/n1', images, meta)
  images2, meta2, _ = raw_utils.load_raw_dataset('train', str(tmp_path), names, 97., 2, 'cuda')
  _check_dataset_against_golden(g, 'plain/n2', images2, meta2, 2, _np(images))
  srgb = meta['postprocess_fn'](images[0])
  assert np.abs(_np(srgb) - ref.postprocess(_np(images[0]), meta['cam2rgb'][0], meta['exposure'])).max() <= 1e-6      # float32 out

  cfg = _raw_config()
  train = datasets.load_dataset('train', str(tmp_path), cfg, device='cuda')
  test = datasets.load_dataset('test', str(tmp_path), cfg, device='cuda')
  assert train.size == 4 and test.size == 1 and (train.height, train.width) == (12, 16)        # llffhold = 8: image 0 is held out
  assert np.array_equal(_np(train.images), g['plain/n1/images'][1:]) and np.array_equal(_np(test.images), g['plain/n1/images'][:1])
  assert np.array_equal(train.metadata['exposure_idx'], g['plain/n1/exposure_idx'][1:])
  b = next(train)
  r = b.rays
  cam = _np(r.cam_idx)[:, 0]
  assert r.exposure_idx.dtype == torch.int32 and r.exposure_idx.shape == (64, 1) and r.exposure_values.shape == (64, 1)
  assert np.array_equal(_np(r.exposure_idx)[:, 0], g['plain/n1/exposure_idx'][1:][cam])
  assert np.array_equal(_np(r.exposure_values)[:, 0], g['plain/n1/exposure_values'][1:][cam].astype(np.float32))
  assert r.lossmult.shape == (64, 3) and (_np(r.lossmult).sum(-1) == 1).all()
  tb = next(test)
  assert tb.rays.exposure_idx.shape == (12, 16, 1) and (_np(tb.rays.exposure_idx) == g['plain/n1/exposure_idx'][0]).all()
  assert tb.rays.lossmult.shape == (12, 16, 1) and tb.rgb.shape == (12, 16, 3)

  # the deferred path keeps the fields, and its Bayer mask is that of its pixels
  cfg2 = _raw_config(['Config.cast_rays_in_train_step = True'])
  pix = next(datasets.load_dataset('train', str(tmp_path), cfg2, device='cuda')).rays
  assert hasattr(pix, 'pix_x_int') and pix.exposure_idx.shape == (64, 1) and pix.exposure_values.shape == (64, 1)
  assert torch.equal(pix.lossmult, raw_utils.pixels_to_bayer_mask(pix.pix_x_int, pix.pix_y_int))
  cam = _np(pix.cam_idx)[:, 0]
  assert np.array_equal(_np(pix.exposure_idx)[:, 0], g['plain/n1/exposure_idx'][1:][cam])
  # the train split of a raw scene stays at full resolution, the test split follows Config.factor
  cfg3 = _raw_config(['Config.factor = 2'])
  cfg3 = dataclasses.replace(cfg3, factor=2)
  assert datasets.load_dataset('train', str(tmp_path), cfg3, device='cuda').images.shape == (4, 12, 16, 3)
  t3 = datasets.load_dataset('test', str(tmp_path), cfg3, device='cuda')
  assert t3.images.shape == (1, 6, 8, 3) and np.array_equal(_np(t3.images), _np(images2[:1]))
  # a render path takes camera 0's exposure
  cfg4 = _raw_config(['Config.render_path = True', 'Config.render_path_frames = 3'])
  rp = datasets.load_dataset('test', str(tmp_path), cfg4, device='cuda')
  rb = rp.generate_ray_batch(2)
  assert rb.rgb is None and (_np(rb.rays.exposure_idx) == g['plain/n1/exposure_idx'][0]).all()
  assert (_np(rb.rays.exposure_values) == np.float32(g['plain/n1/exposure_values'][0])).all()


def test_llff_raw_test_scene_dataset(g, tmp_path):
  rs = np.random.default_rng(2)
  names = ref.write_test_scene(g, str(tmp_path), rs)
  for split in ('train', 'test'):
    images, meta, testscene = raw_utils.load_raw_dataset(split, str(tmp_path), names, 97., 1, 'cuda')
    assert testscene
    _check_dataset_against_golden(g, f'testscene/{split}', images, meta)
  cfg = _raw_config()
  train = datasets.load_dataset('train', str(tmp_path), cfg, device='cuda')
  test = datasets.load_dataset('test', str(tmp_path), cfg, device='cuda')
  assert train.size == 4 and test.size == 1                    # every image of a test scene's split is used
  assert np.array_equal(_np(train.images), g['testscene/train/images']) and np.array_equal(_np(test.images), g['testscene/test/images'])
  assert train.camtoworlds.shape == (4, 3, 4) and test.camtoworlds.shape == (1, 3, 4)
  assert np.array_equal(train.metadata['exposure_idx'], g['testscene/train/exposure_idx'])


def test_procedural_raw_dataset():
  cfg = configs.load_preset('llff_raw', ["Config.dataset_loader = 'procedural'", 'Config.forward_facing = False', 'Config.near = 2.',
                                         'Config.far = 6.', 'Config.factor = 2', 'Config.batch_size = 256'])
  train = datasets.load_dataset('train', None, cfg, device='cuda')
  test = datasets.load_dataset('test', None, cfg, device='cuda')
  S = datasets.Procedural.SIZE
  assert train.images.shape == (40, S, S, 3) and test.images.shape == (6, S // 2, S // 2, 3)
  assert (train.height, train.width, test.height, test.width) == (S, S, S // 2, S // 2) and test.focal == train.focal / 2
  assert len(train.metadata['unique_shutters']) == 3 and len(test.metadata['unique_shutters']) == 1
  assert np.array_equal(train.metadata['exposure_idx'][:6], [0, 1, 2, 0, 1, 2])
  assert np.array_equal(train.metadata['exposure_values'][:3], [1., .5, .25])
  b = next(train)
  r = b.rays
  assert r.lossmult.shape == (256, 3) and r.exposure_idx.shape == (256, 1) and b.rgb.shape == (256, 3)
  # the colour of a train pixel at its Bayer site is the normalised mosaic value itself
  cfg_p = dataclasses.replace(cfg, cast_rays_in_train_step=True)
  tp = datasets.load_dataset('train', None, cfg_p, device='cuda')
  bp = next(tp)
  x, y, cam = (_np(v).reshape(-1).astype(np.int64) for v in (bp.rays.pix_x_int, bp.rays.pix_y_int, bp.rays.cam_idx))
  mask = _np(bp.rays.lossmult)
  assert np.array_equal(mask, _np(raw_utils.pixels_to_bayer_mask(bp.rays.pix_x_int, bp.rays.pix_y_int)))
  mosaics = tp.raw_mosaics
  assert mosaics.dtype == np.uint16 and mosaics.shape == (40, S, S)
  want = ((mosaics[cam, y, x].astype(np.float64) - 64.) / (1023. - 64.)).astype(np.float32)
  assert np.array_equal((_np(bp.rgb) * mask).sum(-1), want)


# ----------------------------------------------------------------------------- image.evaluate_image


@pytest.mark.parametrize('affine', [False, True])
def test_evaluate_image_with_a_postprocess_fn(g, affine):
  """eval.py:118-146 for a raw rendering, restated in NumPy float64: the colour match in raw space (quadratic, or affine
  with Config.eval_raw_affine_cc), then the post-processing of rendering, match and ground truth, 8-bit rounding, crop,
  PSNR and SSIM."""
  cam2rgb, exposure = g['post/cam2rgb'], 0.35
  gt = np.abs(g['post/75x93/raw']).astype(np.float32)
  rs = np.random.default_rng(12)
  est = (gt * np.array([1.2, 0.9, 1.1]) + np.array([0.01, 0.02, -0.005]) + 0.01 * rs.normal(size=gt.shape)).astype(np.float32)
  pp = lambda z: raw_utils.postprocess_raw(z, cam2rgb, exposure)
  config = dataclasses.replace(configs.Config(), eval_quantize_metrics=True, eval_crop_borders=5, eval_raw_affine_cc=affine)
  rendering = {'rgb': _dev(est)}
  batch = types.SimpleNamespace(rgb=_dev(gt))
  metric, metric_cc, images = image.evaluate_image(rendering, batch, config, image.MetricHarness(), postprocess_fn=pp)
  est64, gt64 = est.astype(np.float64), gt.astype(np.float64)
  cc = ref.match_affine(est64, gt64) if affine else image_ref.color_correct(est64, gt64)
  rpp = lambda z: ref.postprocess(z, cam2rgb, exposure)
  want = image_ref.metric_harness(rpp(est64), rpp(gt64), quantize=True, crop=5, cast_f32=True)
  want_cc = image_ref.metric_harness(rpp(cc), rpp(gt64), quantize=True, crop=5, cast_f32=True)
  for name, m, wnt in (('', metric, want), ('cc ', metric_cc, want_cc)):
    for k in ('psnr', 'ssim'):
      print(f'affine {affine}: {name}{k} {m[k]:.12g} reference order {wnt[k]:.12g}')
    assert abs(m['psnr'] - wnt['psnr']) <= PSNR_BOUND and abs(m['ssim'] - wnt['ssim']) <= SSIM_BOUND
  assert want_cc['psnr'] > want['psnr'] + 3                                          # the match does its work
  assert images['color'].dtype == torch.float64 and np.abs(_np(images['color']) - rpp(est64)).max() <= POST_BOUND
  assert np.abs(_np(images['color_cc']) - rpp(cc)).max() <= 1e-10                     # (through the match: conditioning of its sums)
  assert np.abs(_np(rendering['rgb_cc']) - cc).max() <= 1e-10                         # rendering['rgb_cc'] stays in raw space
  with pytest.raises(ValueError, match='eval_raw_affine_cc = True is not supported'):
    image.evaluate_image({'rgb': _dev(est)}, batch, dataclasses.replace(config, eval_raw_affine_cc=True))
