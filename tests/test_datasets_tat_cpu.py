"""The Tanks and Temples loaders, the Blender TIFF inputs and the `tat` preset on the CPU (device='cpu': image.ingest's NumPy
path), on trees the tests write from cameras they chose; and the C ABI's new symbol.  Every test fails without the loaders."""

import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from multinerf_amd import _lib as L
from multinerf_amd import camera_utils, configs, datasets, image, utils
from tests import tat_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOCAL = 24, 32, 40.


def _tat_config(extra=()):
  return configs.load_preset('360+tat', ['Config.batch_size = 64'] + list(extra))


# ----------------------------------------------------------------------------- NeRF++ layout


def test_nerfpp_loader_cameras_images_and_file_order(tmp_path):
  root = str(tmp_path)
  c2w = scenes.ring_cameras(8, seed=1)
  pixels = scenes.random_images(8, H, W, seed=1)
  names = ['f_03', 'a_11', 'z_00', 'b_07', 'm_05', 'c_02', 'k_09', 'd_01']          # written in this order, read sorted
  scenes.write_nerfpp_split(root, 'train', names, c2w, FOCAL, pixels)
  order = np.argsort(names)
  ds = datasets.load_dataset('train', root, _tat_config(['Config.cast_rays_in_train_step = True']), device='cpu')
  assert isinstance(ds, datasets.TanksAndTemplesNerfPP) and ds.size == 8 and (ds.height, ds.width) == (H, W)
  assert ds.images.dtype == torch.float32 and np.array_equal(ds.images.numpy(), pixels[order].astype(np.float32) / np.float32(255.))
  # the files hold c2w diag(1,-1,-1,1) with 17 significant digits (exact); the loader multiplies it back
  assert np.array_equal(ds.camtoworlds.numpy(), c2w[order][:, :3, :4].astype(np.float32))
  assert ds.focal == FOCAL + order[0]                                               # the first SORTED file's focal length
  assert np.array_equal(ds.pixtocams.numpy(), camera_utils.get_pixtocam(ds.focal, W, H).numpy())
  b = next(ds)
  cam = b.rays.cam_idx[:, 0].long()
  assert b.rgb.shape == (64, 3) and torch.equal(b.rgb, ds.images[cam, b.rays.pix_y_int, b.rays.pix_x_int])
  assert float(b.rays.near[0]) == float(np.float32(0.1)) and float(b.rays.far[0]) == 1e6


def test_nerfpp_camera_path_takes_its_resolution_from_the_test_images(tmp_path):
  root = str(tmp_path)
  scenes.write_nerfpp_split(root, 'test', ['0', '1'], scenes.ring_cameras(2), FOCAL, scenes.random_images(2, 10, 14))
  path = scenes.ring_cameras(5, radius=2.0, seed=3)
  scenes.write_nerfpp_split(root, 'camera_path', [f'{i:03d}' for i in range(5)], path, 33.)      # no rgb files
  ds = datasets.load_dataset('test', root, _tat_config(['Config.render_path = True']), device='cpu')
  assert ds.images is None and ds.size == 5 and (ds.height, ds.width) == (10, 14) and ds.focal == 33.
  np.testing.assert_allclose(ds.camtoworlds.numpy(), path[:, :3, :4], atol=1e-6)
  ds._cast_rays_in_train_step, ds.split = True, 'train'                             # (rays need the device: take the pixel form)
  b = ds.generate_ray_batch(3)
  assert isinstance(b.rays, utils.Pixels) and b.rgb is None and b.disps is None and b.normals is None      # rays only
  assert b.rays.pix_x_int.shape == (10, 14) and int(b.rays.cam_idx[0, 0, 0]) == 3


# ----------------------------------------------------------------------------- Free View Synthesis layout


def _fvs_scene(root):
  c2w = scenes.ring_cameras(9, seed=4)
  big, small = scenes.random_images(9, H, W, seed=2), scenes.random_images(9, H // 2, W // 2, seed=3)
  scenes.write_fvs_size(root, 'ibr3d_pw_0.25', c2w, FOCAL / 2, small)
  scenes.write_fvs_size(root, 'ibr3d_pw_0.50', c2w, FOCAL, big)
  os.makedirs(os.path.join(root, 'dense', 'other'))                                  # (not an ibr3d directory)
  w2c = np.linalg.inv(c2w @ scenes.FLIP)[:, :3, :4]
  converted = np.linalg.inv(camera_utils.pad_poses(w2c))[:, :3, :4] @ np.diag([1., -1., -1., 1.])
  np.testing.assert_allclose(converted, c2w[:, :3, :4], atol=1e-12)
  return c2w, big, small, camera_utils.transform_poses_pca(converted)[0]


def test_fvs_loader_poses_split_and_factor(tmp_path):
  root = str(tmp_path)
  c2w, big, small, want_poses = _fvs_scene(root)
  cfg = _tat_config(["Config.dataset_loader = 'tat_fvs'", 'Config.factor = 0', 'Config.llffhold = 4'])
  tr, te = (datasets.load_dataset(s, root, cfg, device='cpu') for s in ('train', 'test'))
  assert isinstance(tr, datasets.TanksAndTemplesFVS)
  test_idx, train_idx = [0, 4, 8], [1, 2, 3, 5, 6, 7]                                # every llffhold-th image, as for LLFF
  assert te.size == 3 and tr.size == 6 and (tr.height, tr.width) == (H, W) and tr.focal == FOCAL      # reversed order: 0.50 first
  np.testing.assert_allclose(tr.poses, want_poses, atol=1e-12)
  assert np.array_equal(tr.camtoworlds.numpy(), want_poses[train_idx][:, :3, :4].astype(np.float32))
  assert np.array_equal(te.camtoworlds.numpy(), want_poses[test_idx][:, :3, :4].astype(np.float32))
  assert np.array_equal(tr.images.numpy(), big[train_idx].astype(np.float32) / np.float32(255.))
  assert np.array_equal(te.images.numpy(), big[test_idx].astype(np.float32) / np.float32(255.))
  assert np.array_equal(tr.pixtocams.numpy(), camera_utils.get_pixtocam(FOCAL, W, H).numpy())
  half = datasets.load_dataset('test', root, dataclasses.replace(cfg, factor=1), device='cpu')
  assert (half.height, half.width) == (H // 2, W // 2) and half.focal == FOCAL / 2
  assert np.array_equal(half.images.numpy(), small[test_idx].astype(np.float32) / np.float32(255.))
  with pytest.raises(ValueError, match='Factor 2 larger than 2'):
    datasets.load_dataset('train', root, dataclasses.replace(cfg, factor=2), device='cpu')


def test_fvs_render_path_test_split_is_an_ellipse_without_images(tmp_path):
  root = str(tmp_path)
  _, _, _, want_poses = _fvs_scene(root)
  cfg = _tat_config(["Config.dataset_loader = 'tat_fvs'", 'Config.factor = 0', 'Config.render_path = True',
                     'Config.render_path_frames = 7', 'Config.z_variation = 0.1', 'Config.z_phase = 0.25'])
  te = datasets.load_dataset('test', root, cfg, device='cpu')
  assert te.images is None and te.size == 7 and (te.height, te.width) == (H, W)
  want = camera_utils.generate_ellipse_path(want_poses, 7, z_variation=0.1, z_phase=0.25)
  assert np.array_equal(te.camtoworlds.numpy(), np.asarray(want)[:, :3, :4].astype(np.float32))
  tr = datasets.load_dataset('train', root, cfg, device='cpu')                       # the train split keeps its images
  assert tr.images is not None and tr.size == 7                                      # llffhold 8 of 9 images: 0 and 8 held out


# ----------------------------------------------------------------------------- Blender TIFF inputs


def _block_mean_f32(x, n):
  """float32 of the float64 block mean added row by row (dy outer, dx inner): mnr_image_ingest's float32 rule."""
  if n == 1:
    return x.astype(np.float32)
  h, w = x.shape[1] // n, x.shape[2] // n
  acc = np.zeros((x.shape[0], h, w) + x.shape[3:], np.float64)
  for dy in range(n):
    for dx in range(n):
      acc += x[:, dy:h * n:n, dx:w * n:n]
  return (acc / np.float64(n * n)).astype(np.float32)


def _srgb_f32(lin):
  eps = np.float32(np.finfo(np.float32).eps)
  s0 = np.float32(323 / 25) * lin
  s1 = (np.float32(211) * np.maximum(lin, eps)**np.float32(5 / 12) - np.float32(11)) / np.float32(200)
  return np.where(lin <= np.float32(0.0031308), s0, s1).astype(np.float32)


@pytest.mark.parametrize('factor', [1, 2, 5])
def test_blender_use_tiffs_equals_the_float32_restatement(tmp_path, factor):
  root = str(tmp_path)
  wrote = scenes.write_blender_scene(root, n=3, size=12, tiffs=True)
  cfg = configs.load_preset('blender_256', ['Config.use_tiffs = True', f'Config.factor = {factor}', 'Config.batch_size = 16'])
  ds = datasets.load_dataset('train', root, cfg, device='cpu')
  size = 12 // factor                                                                # (5 does not divide 12: cropped to 10)
  lin = _block_mean_f32(wrote['train']['linear'], factor)
  assert ds.images.shape == (3, size, size, 3) and lin.shape == (3, size, size, 4)
  srgba = image.linear_to_srgb(torch.from_numpy(lin)).numpy()                        # all four channels, alpha included
  want = srgba[..., :3] * srgba[..., 3:] + (np.float32(1.) - srgba[..., 3:])
  assert np.array_equal(ds.images.numpy(), want)
  # the same in NumPy alone: its float32 pow may differ from torch's in the last place, which the composite passes on
  s = _srgb_f32(lin)
  np.testing.assert_allclose(ds.images.numpy(), s[..., :3] * s[..., 3:] + (np.float32(1.) - s[..., 3:]), atol=4 * 2.0**-24)
  assert (lin <= 0.0031308).any() and (lin > 0.0031308).any()                        # both branches of the curve


@pytest.mark.parametrize('factor', [1, 2])
def test_blender_disparity_maps_fill_batch_disps(tmp_path, factor):
  root = str(tmp_path)
  wrote = scenes.write_blender_scene(root, n=3, size=12, disps=True)
  cfg = configs.load_preset('blender_256', ['Config.compute_disp_metrics = True', f'Config.factor = {factor}', 'Config.batch_size = 16',
                                            'Config.cast_rays_in_train_step = True'])
  ds = datasets.load_dataset('train', root, cfg, device='cpu')
  want = _block_mean_f32(wrote['train']['disp'][..., None], factor)[..., 0]
  assert ds.disp_images.shape == (3, 12 // factor, 12 // factor) and np.array_equal(ds.disp_images.numpy(), want)
  b = next(ds)
  cam = b.rays.cam_idx[:, 0].long()
  assert b.disps.shape == (16,) and torch.equal(b.disps, ds.disp_images[cam, b.rays.pix_y_int, b.rays.pix_x_int])
  # the PNG colours next to it are what they were: bytes / 255 over white
  v = _block_mean_u8(wrote['train']['rgba'], factor) / np.float32(255.)
  assert np.array_equal(ds.images.numpy(), v[..., :3] * v[..., 3:] + (np.float32(1.) - v[..., 3:]))


def _block_mean_u8(x, n):
  """image.downsample of the float32 image, as the loaders wrote it: NumPy's float32 mean over the blocks."""
  a = x.astype(np.float32)
  return a.reshape(a.shape[0], a.shape[1] // n, n, a.shape[2] // n, n, -1).mean((2, 4))


def test_image_ingest_host_path_equals_the_reference_expressions():
  """device='cpu': uint8 plain / white_bg / normals at factors 1, 2, 3 and a cropped 5, against NumPy's float32 mean, `/ 255.`,
  `rgb * alpha + (1. - alpha)` and `x * 2. / 255. - 1.`."""
  x = scenes.random_images(2, 12, 18, 4, seed=5)
  x[0, :5, :5], x[1, -5:, -5:] = 0, 255
  for n in (1, 2, 3, 5):
    xc = x[:, :12 // n * n, :18 // n * n]
    m = _block_mean_u8(xc, n)
    v = m / 255.
    assert v.dtype == np.float32
    assert np.array_equal(image.ingest(x, n, 'plain', 'cpu').numpy(), v)
    assert np.array_equal(image.ingest(x, n, 'plain', 'cpu', c_out=3).numpy(), v[..., :3])
    rgb, alpha = image.ingest(x, n, 'white_bg', 'cpu')
    assert np.array_equal(rgb.numpy(), v[..., :3] * v[..., 3:] + (1. - v[..., 3:])) and np.array_equal(alpha.numpy(), v[..., 3])
    assert np.array_equal(image.ingest(x, n, 'normals', 'cpu').numpy(), m[..., :3] * 2. / 255. - 1.)
  with pytest.raises(ValueError, match='RGBA'):
    image.ingest(x[..., :3], 1, 'white_bg', 'cpu')
  with pytest.raises(ValueError, match='uint8'):
    image.ingest(x.astype(np.float32), 1, 'normals', 'cpu')
  with pytest.raises(ValueError, match='larger than the image'):
    image.ingest(x, 13, 'plain', 'cpu')


# ----------------------------------------------------------------------------- preset, loader table, symbols


def test_tat_preset_and_loader_table():
  cfg = configs.load_preset('360+tat', [])
  assert cfg.dataset_loader == 'tat_nerfpp' and cfg.near == 0.1 and cfg.far == 1e6
  assert configs.load_preset('360', []).dataset_loader != 'tat_nerfpp'
  assert datasets.dataset_dict['tat_nerfpp'] is datasets.TanksAndTemplesNerfPP
  assert datasets.dataset_dict['tat_fvs'] is datasets.TanksAndTemplesFVS and 'dtu' not in datasets.dataset_dict


def test_header_bindings_and_all_three_libraries_agree_on_mnr_image_ingest():
  from tests import sim_helpers
  missing = [os.path.basename(p) for p in (L.LIB_PATH, L.LIB_F32_PATH) if not os.path.exists(p)]
  if missing:
    pytest.skip(f'{", ".join(missing)} not built')
  assert 'mnr_image_ingest' in L.header_symbols() and 'mnr_image_ingest' in L._PROTOS
  assert len(L._PROTOS['mnr_image_ingest'][0]) == 12
  from multinerf_amd import build
  assert 'ingest.hip' in build.SOURCES and 'ingest.hip' in build.SOURCES_F32
  libs = [ctypes.CDLL(L.LIB_PATH), ctypes.CDLL(L.LIB_F32_PATH), sim_helpers.load_sim()]
  for lib in libs:
    assert hasattr(lib, 'mnr_image_ingest')
    lib.mnr_abi_version.restype = ctypes.c_int
    assert lib.mnr_abi_version() == 21
  with open(L.HEADER_PATH) as f:
    header = f.read()
  assert re.search(r'MNR_IMG_U8 = 0, MNR_IMG_F32 = 1', header) and L.IMG_DTYPE == {'uint8': 0, 'float32': 1}
  assert re.search(r'MNR_INGEST_PLAIN = 0, MNR_INGEST_WHITE_BG = 1, MNR_INGEST_NORMALS = 2', header)
  assert L.INGEST_MODE == {'plain': 0, 'white_bg': 1, 'normals': 2}
