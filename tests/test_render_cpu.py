"""Render paths on the CPU: the path generators of multinerf_amd/camera_utils.py against the reference's recorded outputs
(tests/golden/render_path.npz, made by tests/golden/make_golden_render.py; both sides float64 NumPy / FITPACK: atol 1e-9),
the float64 restatements of tests/render_ref.py against the same records (the GPU tests lean on them), and the dataset
loaders with Config.render_path on synthetic COLMAP and NGP scenes."""

import json
import os
import struct

import numpy as np
import pytest
import torch

from multinerf_amd import camera_utils, configs, datasets
from tests import render_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-9


@pytest.fixture(scope='module')
def g():
  return np.load(os.path.join(ROOT, 'tests', 'golden', 'render_path.npz'))


# ----------------------------------------------------------------------------- generators


def test_spiral_path_equals_the_reference(g):
  out = camera_utils.generate_spiral_path(g['spiral/poses'], g['spiral/bounds'], n_frames=7)
  assert out.shape == (7, 3, 4) and out.dtype == np.float64
  np.testing.assert_allclose(out, g['spiral/out'], rtol=0, atol=ATOL)
  out = camera_utils.generate_spiral_path(g['spiral/poses'], g['spiral/bounds'], n_frames=7, n_rots=1, zrate=0.25)
  np.testing.assert_allclose(out, g['spiral/out_rots'], rtol=0, atol=ATOL)
  assert (camera_utils.NEAR_STRETCH, camera_utils.FAR_STRETCH, camera_utils.FOCUS_DISTANCE) == (.9, 5., .75)


@pytest.mark.parametrize('const_speed,key', [(True, 'out_const'), (False, 'out_plain')])
def test_ellipse_path_equals_the_reference(g, const_speed, key):
  out = camera_utils.generate_ellipse_path(g['ellipse/poses'], n_frames=8, const_speed=const_speed, z_variation=0.3, z_phase=0.25)
  assert out.shape == (8, 3, 4)
  np.testing.assert_allclose(out, g[f'ellipse/{key}'], rtol=0, atol=ATOL)


def test_ellipse_path_defaults_and_the_resampling_moves_the_cameras(g):
  out = camera_utils.generate_ellipse_path(g['ellipse/poses'], n_frames=8)
  np.testing.assert_allclose(out, g['ellipse/out_flat'], rtol=0, atol=ATOL)
  assert np.abs(out[:, 2, 3]).max() == 0.0                                       # z_variation = 0: the path lies in z = 0
  assert np.abs(g['ellipse/out_const'] - g['ellipse/out_plain']).max() > 1e-3    # (the fixture tells the two branches apart)


def test_inverse_cdf_resampling_is_the_deterministic_sample():
  """Equal weights: the inverse CDF is the identity on the knots' range, up to the eps the last u stops short of 1 by."""
  t = np.linspace(0, 2 * np.pi, 9)
  out = camera_utils._invert_step_cdf(t, np.zeros(8), 9)
  np.testing.assert_allclose(out, np.linspace(0, 1 - ref.F32_EPS, 9) * 2 * np.pi, rtol=0, atol=1e-12)
  # a zero-width mass: bins of weight ~0 are stepped over
  out = camera_utils._invert_step_cdf(np.array([0., 1., 2., 3.]), np.log(np.array([0.5, 1e-300, 0.5])), 5)
  assert out[2] == pytest.approx(1.0, abs=1e-6) or out[2] == pytest.approx(2.0, abs=1e-6)
  assert np.all(np.diff(out) >= 0) and out[0] == 0.0 and out[-1] <= 3.0


def test_interpolated_path_equals_the_reference(g):
  out = camera_utils.generate_interpolated_path(g['interp/poses'], n_interp=5, spline_degree=5, smoothness=.03, rot_weight=.1)
  assert out.shape == (15, 3, 4)                                                 # degree 5 falls back to n - 1 = 3
  np.testing.assert_allclose(out, g['interp/out'], rtol=0, atol=ATOL)
  out = camera_utils.generate_interpolated_path(g['interp/poses7'], n_interp=3)
  assert out.shape == (18, 3, 4)
  np.testing.assert_allclose(out, g['interp/out7'], rtol=0, atol=ATOL)
  rot = out[:, :, :3]
  np.testing.assert_allclose(np.einsum('nij,nik->njk', rot, rot), np.broadcast_to(np.eye(3), (18, 3, 3)), atol=1e-12)


def test_interpolate_1d_equals_the_reference(g):
  np.testing.assert_allclose(camera_utils.interpolate_1d(g['interp1d/x'], 4, spline_degree=5, smoothness=20), g['interp1d/out'],
                             rtol=0, atol=ATOL)
  out = camera_utils.interpolate_1d(g['interp1d/x'], 3, spline_degree=3, smoothness=0.05)
  assert out.shape == (24,)
  np.testing.assert_allclose(out, g['interp1d/out_k3'], rtol=0, atol=ATOL)


# ----------------------------------------------------------------------------- the restatements the GPU tests use


@pytest.mark.parametrize('tag', ['wp_a', 'wp_b', 'wp_triplet', 'wp_tied', 'wp_zero'])
def test_weighted_percentile_restatement_equals_the_reference(g, tag):
  out = ref.weighted_percentile(g[f'{tag}/x'], g[f'{tag}/w'], g[f'{tag}/ps'])
  np.testing.assert_allclose(out, g[f'{tag}/out'], rtol=0, atol=1e-12)
  if tag == 'wp_zero':
    assert (out == g['wp_zero/x'].max()).all()                                   # all-zero weights: x[-1]
  if tag == 'wp_tied':
    xs = np.sort(g['wp_tied/x'])
    assert out[0] == xs[2] and out[-1] == xs[-1]      # p = 0: the LAST of the zero-weight values in front, as np.interp has it


def test_cmap_restatement_equals_the_reference(g):
  lut, value, weight = g['lut/turbo'], g['cmap/value'], g['cmap/weight']
  lo, hi = g['cmap/lohi'] + [-ref.F32_EPS, ref.F32_EPS]
  out, _ = ref.visualize_cmap_pixels(value, lo, hi, 'neg_log', lut=lut, acc=weight)
  np.testing.assert_allclose(out, g['cmap/out'], rtol=0, atol=1e-15)
  out, _ = ref.visualize_cmap_pixels(value, 2.5, 5.0, 'neg_log', lut=lut)
  np.testing.assert_allclose(out, g['cmap/out_lohi'], rtol=0, atol=1e-15)
  out, _ = ref.visualize_cmap_pixels(value, 0, 1, None, modulus=0.25, lut=lut, acc=weight)
  np.testing.assert_allclose(out, g['cmap/out_mod'], rtol=0, atol=1e-15)
  lo, hi = g['cmap/lohi3'] + [-ref.F32_EPS, ref.F32_EPS]
  out, _ = ref.visualize_cmap_pixels(g['cmap/value3'], lo, hi, 'log', acc=weight)
  np.testing.assert_allclose(out, g['cmap/out_c3'], rtol=0, atol=1e-15)


def test_suite_restatements_equal_the_reference(g):
  gin = lambda k: g[f'suite/in/{k}']
  acc = np.where(np.isnan(gin('distance_mean')), 0.0, gin('acc'))
  np.testing.assert_array_equal(g['suite/out/acc'], acc)
  np.testing.assert_allclose(ref.matte(gin('rgb'), acc), g['suite/out/color_matte'], rtol=0, atol=1e-15)
  np.testing.assert_allclose(ref.matte(ref.preop('half', gin('normals')), acc), g['suite/out/normals'], rtol=0, atol=1e-15)
  np.testing.assert_allclose(ref.matte(ref.preop('tanh', gin('roughness')), acc), g['suite/out/roughness'], rtol=0, atol=1e-15)
  coords = ref.preop('coord_mod', origins=gin('origins'), directions=gin('directions'), distance=gin('distance_mean'))
  np.testing.assert_allclose(ref.matte(coords, acc), g['suite/out/coords_mod'], rtol=0, atol=1e-15, equal_nan=True)


@pytest.mark.parametrize('tag', ['sph_6x9', 'sph_17x32'])
def test_spherical_restatement_equals_the_reference(g, tag):
  H, W = (int(v) for v in tag[4:].split('x'))
  o, d, r = ref.spherical_rays(g[f'{tag}/c2w'], H, W)
  np.testing.assert_array_equal(o, g[f'{tag}/origins'])
  np.testing.assert_allclose(d, g[f'{tag}/directions'], rtol=0, atol=1e-15)
  np.testing.assert_allclose(r, g[f'{tag}/radii'], rtol=0, atol=1e-15)
  assert not g[f'{tag}/imageplane'].any() and g[f'{tag}/imageplane'].shape == (H, W, 2)


# ----------------------------------------------------------------------------- loaders


def _write_colmap_scene(root, n=9, size=(12, 10)):
  """A COLMAP sparse model (published binary layout, OPENCV camera) with PNG images and their half-size copies."""
  from PIL import Image
  rs = np.random.default_rng(1)
  w, h = size
  for d in ('sparse/0', 'images', 'images_2'):
    os.makedirs(os.path.join(root, d), exist_ok=True)
  with open(os.path.join(root, 'sparse/0/cameras.bin'), 'wb') as f:
    f.write(struct.pack('<Q', 1))
    f.write(struct.pack('<iiQQ', 1, 4, w, h))
    f.write(struct.pack('<8d', 50.0, 52.0, w / 2., h / 2., 0.01, -0.002, 0.0005, 0.0003))
  names = []
  with open(os.path.join(root, 'sparse/0/images.bin'), 'wb') as f:
    f.write(struct.pack('<Q', n))
    for i in range(n):
      q = rs.normal(size=4)
      q /= np.linalg.norm(q)
      name = f'img_{n - i:02d}.png'
      f.write(struct.pack('<i7di', i + 1, *q, *rs.normal(size=3), 1))
      f.write(name.encode() + b'\x00')
      f.write(struct.pack('<Q', 0))
      names.append(name)
      Image.fromarray(rs.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, 'images', name))
      Image.fromarray(rs.integers(0, 256, (h // 2, w // 2, 3), dtype=np.uint8)).save(os.path.join(root, 'images_2', name))
  return names


def _write_ngp_scene(root, n=8):
  """An NGP transforms.json scene of nearly parallel cameras, with poses_bounds.npy."""
  from PIL import Image
  rs = np.random.default_rng(2)
  os.makedirs(os.path.join(root, 'images'))
  frames = []
  for i in range(n):
    Image.fromarray(rs.integers(0, 256, (6, 8, 3), dtype=np.uint8)).save(os.path.join(root, 'images', f'{i}.png'))
    m = np.eye(4)
    m[:3, :3] += 0.05 * rs.normal(size=(3, 3))
    m[:3, 3] = rs.normal(size=3) * 0.3
    frames.append({'file_path': f'images/{i}.png', 'transform_matrix': m.tolist()})
  json.dump({'w': 8, 'h': 6, 'fl_x': 10.0, 'fl_y': 10.0, 'frames': frames}, open(os.path.join(root, 'transforms.json'), 'w'))
  bounds = np.concatenate([np.zeros((n, 15)), rs.uniform(2.0, 3.0, (n, 1)), rs.uniform(8.0, 9.0, (n, 1))], 1)
  np.save(os.path.join(root, 'poses_bounds.npy'), bounds)
  return bounds[:, -2:]


_RENDER = ['Config.render_path = True', 'Config.render_path_frames = 6']


def test_llff_ellipse_render_path(tmp_path):
  root = str(tmp_path)
  _write_colmap_scene(root)
  cfg = configs.load_preset('360', ['Config.factor = 2', 'Config.z_variation = 0.2', 'Config.z_phase = 0.1',
                                    'Config.render_resolution = (16, 10)', 'Config.render_focal = 20.0'] + _RENDER)
  ds = datasets.load_dataset('test', root, cfg, device='cpu')
  assert ds.size == 6 and ds.render_path
  want = camera_utils.generate_ellipse_path(ds.poses, n_frames=6, z_variation=0.2, z_phase=0.1)
  assert ds.poses.shape == (9, 3, 4)                                              # the path is built on all poses, not on the split's
  np.testing.assert_allclose(ds.camtoworlds.numpy(), want, rtol=0, atol=1e-6)    # (float32 storage)
  assert (ds.width, ds.height, ds.focal) == (16, 10, 20.0)
  np.testing.assert_allclose(ds.pixtocams.numpy(), np.linalg.inv(np.array([[20., 0, 8.], [0, 20., 5.], [0, 0, 1.]])), atol=1e-7)
  assert ds.distortion_params is None and ds.cameras[2] is None
  assert ds.camtype == camera_utils.ProjectionType.PERSPECTIVE and not ds._render_spherical
  # without render_resolution / render_focal the loader's own intrinsics stay, without distortion
  cfg = configs.load_preset('360', ['Config.factor = 2'] + _RENDER)
  ds = datasets.load_dataset('test', root, cfg, device='cpu')
  assert (ds.width, ds.height) == (6, 5) and ds.distortion_params is None
  np.testing.assert_allclose(ds.pixtocams.numpy(), np.linalg.inv(np.array([[25., 0, 3.], [0, 25., 2.5], [0, 0, 1.]])), atol=1e-7)


def test_llff_spline_render_path_from_a_text_file(tmp_path):
  root = str(tmp_path / 'scene')
  names = _write_colmap_scene(root)
  keyfile = str(tmp_path / 'keyframes.txt')
  keys = sorted(names)[1:8:2]                                                      # 4 keyframes
  with open(keyfile, 'w') as f:
    f.write('\n'.join(keys) + '\n')
  cfg = configs.load_preset('360', ['Config.factor = 2', f"Config.render_spline_keyframes = '{keyfile}'",
                                    'Config.render_spline_n_interp = 4'] + _RENDER)
  ds = datasets.load_dataset('test', root, cfg, device='cpu')
  assert list(ds.spline_indices) == [1, 3, 5, 7] and ds.render_exposures is None
  assert ds.size == 4 * 3                                                          # n_interp * (keyframes - 1), not render_path_frames
  want = camera_utils.generate_interpolated_path(ds.poses[[1, 3, 5, 7]], n_interp=4, spline_degree=5, smoothness=.03, rot_weight=.1)
  np.testing.assert_allclose(ds.camtoworlds.numpy(), want, rtol=0, atol=1e-6)
  # a directory of images names the keyframes too
  keydir = str(tmp_path / 'keys')
  os.makedirs(keydir)
  for k in keys:
    open(os.path.join(keydir, k), 'w').close()
  cfg = configs.load_preset('360', ['Config.factor = 2', f"Config.render_spline_keyframes = '{keydir}'",
                                    'Config.render_spline_n_interp = 4'] + _RENDER)
  np.testing.assert_array_equal(datasets.load_dataset('test', root, cfg, device='cpu').camtoworlds.numpy(), ds.camtoworlds.numpy())
  cfg = configs.load_preset('360', ['Config.factor = 2', f"Config.render_spline_keyframes = '{keyfile}'",
                                    'Config.render_spline_interpolate_exposure = True'] + _RENDER)
  with pytest.raises(ValueError, match='exposures=None'):
    datasets.load_dataset('test', root, cfg, device='cpu')


def test_llff_forward_facing_spiral_render_path(tmp_path):
  root = str(tmp_path)
  bounds = _write_ngp_scene(root)
  cfg = configs.load_preset('360', ['Config.factor = 0', 'Config.forward_facing = True'] + _RENDER)
  ds = datasets.load_dataset('test', root, cfg, device='cpu')
  assert ds.size == 6 and ds.pixtocam_ndc is not None
  scale = 1. / (bounds.min() * .75)
  want = camera_utils.generate_spiral_path(ds.poses, bounds * scale, n_frames=6)   # the bounds are scaled with the poses
  np.testing.assert_allclose(ds.camtoworlds.numpy(), want, rtol=0, atol=1e-6)
  unscaled = camera_utils.generate_spiral_path(ds.poses, bounds, n_frames=6)
  assert np.abs(unscaled - want).max() > 1e-3


def test_render_path_file_camtype_and_batches(tmp_path):
  root = str(tmp_path / 'scene')
  _write_colmap_scene(root)
  poses = np.random.default_rng(5).normal(size=(4, 3, 4))
  posefile = str(tmp_path / 'poses.npy')
  np.save(posefile, poses)
  cfg = configs.load_preset('360', ['Config.factor = 2', f"Config.render_path_file = '{posefile}'",
                                    "Config.render_camtype = 'fisheye'"] + _RENDER)
  ds = datasets.load_dataset('test', root, cfg, device='cpu')
  assert ds.size == 4 and ds.camtype == camera_utils.ProjectionType.FISHEYE
  np.testing.assert_allclose(ds.camtoworlds.numpy(), poses, rtol=0, atol=1e-6)
  cfg = configs.load_preset('360', ['Config.factor = 2', "Config.render_camtype = 'pano'"] + _RENDER)
  ds = datasets.load_dataset('test', root, cfg, device='cpu')
  assert ds._render_spherical and ds.camtype == camera_utils.ProjectionType.PERSPECTIVE
  # the train split with cast_rays_in_train_step makes pixel batches without the ray kernel: no rgb under render_path
  cfg = configs.load_preset('360', ['Config.factor = 2', 'Config.cast_rays_in_train_step = True', 'Config.batch_size = 16'] + _RENDER)
  b = next(datasets.load_dataset('train', root, cfg, device='cpu'))
  assert b.rgb is None and b.rays.pix_x_int.shape == (16,)
  # render exposures (set by the spline path with render_spline_interpolate_exposure) feed exposure_values per camera
  cfg = configs.load_preset('360', ['Config.factor = 2', 'Config.cast_rays_in_train_step = True', 'Config.batch_size = 16',
                                    'Config.batching = "single_image"'] + _RENDER)
  tr = datasets.load_dataset('train', root, cfg, device='cpu')
  tr.render_exposures = np.array([0.5, 2.0, 4.0, 1.5, 1.25, 3.0])
  px = torch.zeros(5, dtype=torch.int64)
  b = tr._make_ray_batch(px, px, 2)
  assert b.rays.exposure_values.shape == (5, 1) and (b.rays.exposure_values == 4.0).all()


def test_procedural_render_path_and_blender_refusal(tmp_path):
  cfg = configs.load_preset('blender_256', ["Config.dataset_loader = 'procedural'", 'Config.z_variation = 0.5'] + _RENDER)
  ds = datasets.load_dataset('test', None, cfg, device='cpu')
  plain = datasets.load_dataset('test', None, configs.load_preset('blender_256', ["Config.dataset_loader = 'procedural'"]), device='cpu')
  want = camera_utils.generate_ellipse_path(plain.camtoworlds.numpy().astype(np.float64), n_frames=6, z_variation=0.5)
  assert ds.size == 6
  np.testing.assert_allclose(ds.camtoworlds.numpy(), want, rtol=0, atol=1e-5)
  centres = ds.camtoworlds.numpy()[:, :, 3]
  assert 2.0 < np.linalg.norm(centres, axis=-1).min() and np.linalg.norm(centres, axis=-1).max() < 6.0   # inside near / far of the scene
  with pytest.raises(ValueError, match='render_path cannot be used for the blender dataset'):
    datasets.Blender('test', str(tmp_path), configs.load_preset('blender_256', _RENDER), device='cpu')
