"""Image ingest on the GPU (-m gpu): csrc/ingest.hip through multinerf_amd.ops / image.ingest against NumPy float32
restatements of the reference's expressions, then the loaders that use it (Blender, LLFF, Tanks and Temples) and two train
steps of the `360+tat` preset.  tests/test_sim_ingest.py runs this file on the kernel-source simulator.

Expected values.
  * uint8: `image.downsample`'s float32 mean over the n x n blocks, `/ 255.`, `rgb * alpha + (1. - alpha)` and
    `x * 2. / 255. - 1.`, written with NumPy in float32: bit-equal (np.array_equal).  The block sum of at most 256 x 256 bytes
    is an integer below 2^24, exact in float32 in any order, so NumPy's mean is float(S) / float(n n) whichever way it adds.
  * float32, n = 1: the input.  n > 1: bit-equal to float32 of the float64 sum added row by row (dy outer, dx inner) and
    divided by n n in float64; and within n^2 2^-24 max|v| of NumPy's float32 mean (n^2 - 1 additions and a division, each
    rounding at 2^-24 of a partial sum of at most n^2 max|v|, over n^2: the bound tests/test_gpu_raw.py derives).
  * Two runs agree bit for bit.
"""

import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import _lib as L
from multinerf_amd import configs, datasets, image, ops, train_utils
from tests import tat_scenes as scenes

SIMULATED = os.environ.get('MNR_TESTS_ON_SIMULATOR') == '1'
# (N, H, W, C, n, C_out)
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 6, 10, 3, 1, 3), (2, 6, 10, 4, 2, 4), (1, 15, 21, 3, 3, 3), (3, 40, 72, 4, 8, 4), (2, 130, 258, 3, 2, 3),
          (1, 7, 1030, 1, 1, 1),                                  # one row wider than a workgroup
          (2, 6, 10, 4, 1, 3)]
IDS = ['x'.join(str(v) for v in s) for s in SHAPES]
F32 = np.float32


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')


def _dev(x):
  return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(t):
  return t.cpu().numpy()


def _bytes(N, H, W, C, n):
  """Random bytes; the first block of the first image is 0 and the last block of the last image 255 in every channel."""
  x = np.random.default_rng([11, N, H, W, C, n]).integers(0, 256, (N, H, W, C), dtype=np.uint8)
  if H * W > n * n:
    x[0, :n, :n] = 0
  x[-1, H - n:, W - n:] = 255
  return x


def _mean_f32(x, n):
  """image.downsample of a float32 image stack: NumPy's float32 mean over the n x n blocks."""
  a = x.astype(F32)
  return a if n == 1 else a.reshape(a.shape[0], a.shape[1] // n, n, a.shape[2] // n, n, a.shape[3]).mean((2, 4))


def _mean_f64_rows(x, n):
  """float32 of the float64 block sum added row by row (dy outer, dx inner), divided by n n in float64: the kernel's order."""
  acc = np.zeros((x.shape[0], x.shape[1] // n, x.shape[2] // n, x.shape[3]), np.float64)
  for dy in range(n):
    for dx in range(n):
      acc += x[:, dy::n, dx::n]
  return (acc / np.float64(n * n)).astype(F32)


# ----------------------------------------------------------------------------- the kernel


@pytest.mark.parametrize('N,H,W,C,n,c_out', SHAPES, ids=IDS)
def test_uint8_modes_are_bit_equal_to_the_float32_expressions(N, H, W, C, n, c_out):
  x = _bytes(N, H, W, C, n)
  xd = _dev(x)
  m = _mean_f32(x, n)
  v = m / 255.
  assert m.dtype == F32 and v.dtype == F32
  got = ops.image_ingest(xd, n, 'plain', c_out)
  assert got.dtype == torch.float32 and tuple(got.shape) == (N, H // n, W // n, c_out)
  assert np.array_equal(_np(got), v[..., :c_out])
  assert _np(got).min() == 0. or H * W <= n * n
  assert _np(got).max() == 1.
  assert torch.equal(ops.image_ingest(xd, n, 'plain', c_out), got)                            # two runs
  if c_out == C and C > 1:                                                                   # a channel subset of the same input
    assert np.array_equal(_np(ops.image_ingest(xd, n, 'plain', 1)), v[..., :1])
  if C == 4:
    rgb, alpha = ops.image_ingest(xd, n, 'white_bg', want_alpha=True)
    want = v[..., :3] * v[..., 3:] + (1. - v[..., 3:])
    assert want.dtype == F32 and tuple(rgb.shape) == (N, H // n, W // n, 3) and tuple(alpha.shape) == (N, H // n, W // n)
    assert np.array_equal(_np(rgb), want) and np.array_equal(_np(alpha), v[..., 3])
    assert torch.equal(ops.image_ingest(xd, n, 'white_bg'), rgb)                              # without alpha; a second run
  if C >= 3:
    nrm = ops.image_ingest(xd, n, 'normals')
    want = m[..., :3] * 2. / 255. - 1.
    assert want.dtype == F32 and np.array_equal(_np(nrm), want) and torch.equal(ops.image_ingest(xd, n, 'normals'), nrm)
    assert _np(nrm).max() == 1. and (_np(nrm).min() == -1. or H * W <= n * n)


@pytest.mark.parametrize('n', [1, 2, 3])
def test_white_background_at_alpha_0_and_255(n):
  x = _bytes(2, 12, 18, 4, n)
  x[0, ..., 3], x[1, ..., 3] = 0, 255
  rgb, alpha = ops.image_ingest(_dev(x), n, 'white_bg', want_alpha=True)
  rgb, alpha = _np(rgb), _np(alpha)
  assert (rgb[0] == 1.).all() and (alpha[0] == 0.).all()                                      # transparent: exactly white
  assert (alpha[1] == 1.).all() and np.array_equal(rgb[1], _mean_f32(x, n)[1, ..., :3] / 255.)   # opaque: exactly rgb / 255


def test_unaligned_source_and_output_take_the_same_values():
  """A source that starts 1 byte past a 4-byte boundary and an output 4 bytes past a 16-byte boundary (the vector paths
  need both aligned): the per-pixel path and the strip path's unaligned ends."""
  for (N, H, W, C, n) in ((2, 6, 10, 3, 1), (2, 6, 10, 4, 1), (2, 6, 10, 4, 2), (1, 15, 21, 3, 3)):
    x = _bytes(N, H, W, C, n)
    flat = _dev(np.concatenate([np.zeros(1, np.uint8), x.reshape(-1)]))
    xd = flat[1:].reshape(N, H, W, C)
    assert xd.data_ptr() % 4 == 1 and xd.is_contiguous()
    count = N * (H // n) * (W // n) * C
    buf = torch.zeros(count + 1, dtype=torch.float32).cuda()
    out = buf[1:]
    got = ops.image_ingest(xd, n, 'plain', out=out)
    assert np.array_equal(_np(got), _mean_f32(x, n) / 255.) and float(buf[0]) == 0.
    if C == 4:
      assert np.array_equal(_np(ops.image_ingest(xd, n, 'white_bg')), _np(ops.image_ingest(_dev(x), n, 'white_bg')))


@pytest.mark.parametrize('N,H,W,C,n,c_out', SHAPES, ids=IDS)
def test_float32_input(N, H, W, C, n, c_out):
  rs = np.random.default_rng([12, N, H, W, C, n])
  x = (rs.uniform(0, 1, (N, H, W, C)) * 10.0**rs.integers(-3, 3, (N, H, W, C))).astype(F32)
  xd = _dev(x)
  got = ops.image_ingest(xd, n, 'plain', c_out)
  assert got.dtype == torch.float32 and torch.equal(ops.image_ingest(xd, n, 'plain', c_out), got)
  if n == 1:
    assert np.array_equal(_np(got), x[..., :c_out])
  else:
    assert np.array_equal(_np(got), _mean_f64_rows(x, n)[..., :c_out])
    bound = n * n * 2.0**-24 * np.abs(x).max()
    diff = np.abs(_np(got).astype(np.float64) - _mean_f32(x, n)[..., :c_out]).max()
    print(f'float32 {N}x{H}x{W}x{C} n={n}: max |diff| to the float32 mean {diff:.3g} (bound {bound:.3g})')
    assert diff <= bound
  if C == 4:                                                                                 # v = m: the composite of float pixels
    rgb, alpha = ops.image_ingest(xd, n, 'white_bg', want_alpha=True)
    v = _mean_f64_rows(x, n) if n > 1 else x
    assert np.array_equal(_np(rgb), v[..., :3] * v[..., 3:] + (F32(1.) - v[..., 3:])) and np.array_equal(_np(alpha), v[..., 3])


def _status(N, H, W, C, dtype, src, n, mode, c_out, out, alpha=None):
  return ops.lib().mnr_image_ingest(N, H, W, C, dtype, ops._ptr(src), n, mode, c_out, ops._ptr(out), ops._ptr(alpha), ops._stream())


def test_argument_errors_return_an_error_and_leave_out_untouched():
  src = _dev(np.full((2, 6, 10, 4), 200, np.uint8))
  srcf = _dev(np.full((2, 6, 10, 4), .5, F32))
  big = _dev(np.full((1, 514, 514, 1), 9, np.uint8))
  out = torch.full((514 * 514,), 7., dtype=torch.float32).cuda()
  U8, F, PLAIN, WHITE, NORMALS = 0, 1, 0, 1, 2
  bad = {
      'dtype 2': (2, 6, 10, 4, 2, src, 1, PLAIN, 4),
      'dtype -1': (2, 6, 10, 4, -1, src, 1, PLAIN, 4),
      'mode 3': (2, 6, 10, 4, U8, src, 1, 3, 3),
      'mode -1': (2, 6, 10, 4, U8, src, 1, -1, 3),
      'C 0': (2, 6, 10, 0, U8, src, 1, PLAIN, 1),
      'C 5': (2, 6, 8, 5, U8, src, 1, PLAIN, 3),
      'C_out 0': (2, 6, 10, 4, U8, src, 1, PLAIN, 0),
      'C_out > C': (2, 6, 20, 2, U8, src, 1, PLAIN, 3),
      'n 0': (2, 6, 10, 4, U8, src, 0, PLAIN, 4),
      'n -2': (2, 6, 10, 4, U8, src, -2, PLAIN, 4),
      'n does not divide H': (2, 6, 10, 4, U8, src, 5, PLAIN, 4),
      'n does not divide W': (2, 6, 10, 4, U8, src, 3, PLAIN, 4),
      'n 257 with uint8': (1, 514, 514, 1, U8, big, 257, PLAIN, 1),
      'white_bg with C 3': (2, 8, 10, 3, U8, src, 1, WHITE, 3),
      'white_bg with C_out 4': (2, 6, 10, 4, U8, src, 1, WHITE, 4),
      'normals with float32': (2, 6, 10, 4, F, srcf, 1, NORMALS, 3),
      'normals with C 2': (2, 6, 20, 2, U8, src, 1, NORMALS, 2),
      'negative N': (-1, 6, 10, 4, U8, src, 1, PLAIN, 4),
  }
  for tag, (N, H, W, C, dtype, s, n, mode, c_out) in bad.items():
    st = _status(N, H, W, C, dtype, s, n, mode, c_out, out)
    assert st == L.MNR_ERR_INVALID_ARGUMENT, tag
    assert ops.lib().mnr_last_error().decode().startswith('mnr_image_ingest:'), tag
  assert _status(0, 6, 10, 4, U8, src, 1, PLAIN, 4, out) == L.MNR_OK                          # N == 0: a successful no-op
  assert _status(0, 6, 10, 4, U8, None, 2, WHITE, 3, None) == L.MNR_OK
  torch.cuda.synchronize()
  assert (_np(out) == 7.).all()
  # n = 256 is the largest uint8 block: 65536 x 200 is exact
  blk = _dev(np.full((1, 256, 512, 1), 200, np.uint8))
  assert np.array_equal(_np(ops.image_ingest(blk, 256)), np.full((1, 1, 2, 1), F32(200) / F32(255)))
  # the wrapper refuses the same, and what is not a device image
  for kw, match in ((dict(n_downsample=4), 'must divide'), (dict(n_downsample=0), 'must divide'), (dict(mode='srgb'), 'must be one of'),
                    (dict(c_out=5), 'c_out'), (dict(c_out=0), 'c_out'), (dict(mode='white_bg', c_out=4), 'white_bg'),
                    (dict(want_alpha=True), 'alpha is an output'), (dict(out=torch.zeros(5).cuda()), 'out ')):
    with pytest.raises(ValueError, match=match):
      ops.image_ingest(src, **kw)
  with pytest.raises(ValueError, match='white_bg'):
    ops.image_ingest(src[..., :3].contiguous(), mode='white_bg')
  with pytest.raises(ValueError, match='normals'):
    ops.image_ingest(srcf, mode='normals')
  with pytest.raises(ValueError, match='> 256'):
    ops.image_ingest(big, 257)
  with pytest.raises(ValueError, match='uint8 or float32'):
    ops.image_ingest(src.to(torch.int32))
  with pytest.raises(ValueError, match='contiguous'):
    ops.image_ingest(src[:, :, ::2])
  with pytest.raises(ValueError, match='1 to 4 channels'):
    ops.image_ingest(_dev(np.zeros((1, 2, 2, 5), np.uint8)))
  if not SIMULATED:                                                                          # (the simulator takes host tensors by design)
    with pytest.raises(ValueError, match='device tensor'):
      ops.image_ingest(torch.zeros((1, 2, 2, 3), dtype=torch.uint8))


# ----------------------------------------------------------------------------- loaders: the device against the host path


def _same(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize('factor', [1, 2, 3])
def test_blender_png_scene_is_the_same_on_the_device_and_on_the_host(tmp_path, factor):
  root = str(tmp_path)
  wrote = scenes.write_blender_scene(root, n=4, size=12)
  cfg = configs.load_preset('blender_256', ['Config.compute_normal_metrics = True', f'Config.factor = {factor}', 'Config.batch_size = 16'])
  dev, host = (datasets.load_dataset('train', root, cfg, device=d) for d in ('cuda', 'cpu'))
  s = 12 // factor
  assert tuple(dev.images.shape) == (4, s, s, 3) and tuple(dev.normal_images.shape) == (4, s, s, 3) and tuple(dev.alphas.shape) == (4, s, s)
  assert _same(dev.images, host.images) and _same(dev.normal_images, host.normal_images) and _same(dev.alphas, host.alphas)
  # and both are what the loader computed before image.ingest existed
  a = _mean_f32(wrote['train']['rgba'], factor) / 255.
  assert np.array_equal(_np(dev.images), a[..., :3] * a[..., 3:] + (1. - a[..., 3:])) and np.array_equal(_np(dev.alphas), a[..., 3])
  assert np.array_equal(_np(dev.normal_images), _mean_f32(wrote['train']['normals'], factor) * 2. / 255. - 1.)
  if not SIMULATED:
    assert dev.images.is_cuda and dev.normal_images.is_cuda


def test_llff_scene_is_the_same_on_the_device_and_on_the_host(tmp_path):
  root = str(tmp_path)
  pixels = scenes.write_llff_scene(root)
  cfg = configs.load_preset('360', ['Config.factor = 0', 'Config.batch_size = 16'])
  for split, idx in (('train', [1, 2, 3, 4, 5, 6, 7]), ('test', [0])):
    dev, host = (datasets.load_dataset(split, root, cfg, device=d) for d in ('cuda', 'cpu'))
    assert _same(dev.images, host.images) and np.array_equal(_np(dev.images), pixels[idx].astype(F32) / 255.)
    assert dev.normal_images is None and dev.alphas is None and host.alphas is None


def test_blender_tiff_and_disparity_inputs_on_the_device(tmp_path):
  root = str(tmp_path)
  wrote = scenes.write_blender_scene(root, n=2, size=12, tiffs=True, disps=True)
  cfg = configs.load_preset('blender_256', ['Config.use_tiffs = True', 'Config.compute_disp_metrics = True', 'Config.factor = 2',
                                            'Config.batch_size = 16'])
  ds = datasets.load_dataset('test', root, cfg, device='cuda')
  assert np.array_equal(_np(ds.disp_images), _mean_f64_rows(wrote['test']['disp'][..., None], 2)[..., 0])
  lin = _mean_f64_rows(wrote['test']['linear'], 2)
  s = _np(image.linear_to_srgb(_dev(lin)))
  assert np.array_equal(_np(ds.images), s[..., :3] * s[..., 3:] + (F32(1.) - s[..., 3:]))
  b = ds.generate_ray_batch(1)
  assert tuple(b.disps.shape) == (6, 6) and torch.equal(b.disps, ds.disp_images[1]) and torch.equal(b.rgb, ds.images[1])


# ----------------------------------------------------------------------------- Tanks and Temples scenes on the device

TAT_N, TAT_H, TAT_W, TAT_FOCAL = 8, 24, 32, 40.
TAT_BINDS = ['NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'Config.batch_size = 1024']


def _write_tat(root, loader):
  c2w = scenes.ring_cameras(TAT_N, seed=6)
  pixels = scenes.random_images(TAT_N, TAT_H, TAT_W, seed=7)
  if loader == 'tat_nerfpp':
    scenes.write_nerfpp_split(root, 'train', [f'{i:04d}' for i in range(TAT_N)], c2w, TAT_FOCAL, pixels)
    return pixels
  scenes.write_fvs_size(root, 'ibr3d_pw_0.50', c2w, TAT_FOCAL, pixels)
  return pixels[np.arange(TAT_N) % 8 != 0]                                                   # llffhold = 8: image 0 is held out


def _tat_config(loader, extra=()):
  binds = TAT_BINDS + ([] if loader == 'tat_nerfpp' else ["Config.dataset_loader = 'tat_fvs'", 'Config.factor = 0'])
  return configs.load_preset('360+tat', binds + list(extra))


@pytest.mark.parametrize('loader', ['tat_nerfpp', 'tat_fvs'])
def test_tat_scene_images_and_train_batches(tmp_path, loader):
  root = str(tmp_path)
  pixels = _write_tat(root, loader)
  ds = datasets.load_dataset('train', root, _tat_config(loader), device='cuda')
  assert ds.size == len(pixels) and (ds.height, ds.width) == (TAT_H, TAT_W) and ds.focal == TAT_FOCAL
  assert ds.images.dtype == torch.float32 and np.array_equal(_np(ds.images), pixels.astype(F32) / 255.)
  b = next(ds)
  r = b.rays
  cam = r.cam_idx[:, 0].long()
  assert tuple(b.rgb.shape) == (1024, 3)
  finite = lambda t: bool(torch.isfinite(t).all())
  assert finite(r.origins) and finite(r.directions) and finite(r.viewdirs) and finite(r.radii)
  assert (_np(r.near) == F32(0.1)).all() and (_np(r.far) == F32(1e6)).all()
  # the colours are those of the pixels the rays were cast through (the deferred form carries the pixel indices)
  pix = next(datasets.load_dataset('train', root, _tat_config(loader, ['Config.cast_rays_in_train_step = True']), device='cuda'))
  cam = pix.rays.cam_idx[:, 0].long()
  assert torch.equal(pix.rgb, ds.images[cam, pix.rays.pix_y_int, pix.rays.pix_x_int])
  assert (_np(pix.rays.near) == F32(0.1)).all() and (_np(pix.rays.far) == F32(1e6)).all()
  assert np.array_equal(_np(pix.rgb), (pixels[_np(cam), _np(pix.rays.pix_y_int), _np(pix.rays.pix_x_int)]).astype(F32) / 255.)


@pytest.mark.parametrize('deferred', [False, True])
@pytest.mark.parametrize('loader', ['tat_nerfpp', 'tat_fvs'])
def test_two_train_steps_of_the_tat_preset(tmp_path, loader, deferred):
  root = str(tmp_path)
  _write_tat(root, loader)
  cfg = _tat_config(loader, [f'Config.cast_rays_in_train_step = {deferred}'])
  ds = datasets.load_dataset('train', root, cfg, device='cuda')
  model, state, _, train_pstep, _ = train_utils.setup_model(cfg, 20200823, dataset=ds, device='cuda')
  gen = torch.Generator(device=ds.images.device).manual_seed(20200823)
  for step in (1, 2):
    state, stats, gen = train_pstep(gen, state, next(ds), ds.cameras, (step - 1) / (cfg.max_steps - 1), 1.0)
    loss = stats.materialize()['loss']
    print(f'{loader} deferred={deferred} step {step}: loss {loss:.6g}')
    assert np.isfinite(loss) and loss > 0
