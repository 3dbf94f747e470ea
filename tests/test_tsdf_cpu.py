"""TSDF fusion, the parts that need no GPU: mesh.world_to_pixel against the oracle's pixels_to_rays and its refusals, the NumPy
restatement (tests/tsdf_ref.py) alone on the analytic sphere scene, the C entries' argument checks, the command line, and
that the new translation unit is listed wherever the others are."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

from multinerf_amd import _lib, build, camera_utils, mesh
from oracle import camera_utils as ocam
from tests import tsdf_ref as T
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_to_pixel_inverts_the_oracles_pixels_to_rays():
  """Points origin + t * direction of the oracle's rays project to the pixel's centre (px + 0.5, py + 0.5) with zc = t.

  Bound.  The oracle runs in float64 and the matrix is formed in float64, so the only float32 rounding is that of the 12 entries
  of P: |dP_rj| <= 2^-24 |P_rj|.  With X the point, m_r = P_r . (X, 1) is then off by at most 2^-24 mag_r, mag_r = sum_j |P_rj|
  |X_j| + |P_r3|.  u = m_0 / zc with zc = t > 0, so |du| <= (|dm_0| + |u| |dzc|) / zc to first order, i.e.
  2^-24 (mag_0 + |u| mag_2) / t, likewise v, and |dzc| <= 2^-24 mag_2.  1 % is added for the second order, 1e-9 (relative to the
  magnitudes) for the float64 arithmetic on both sides."""
  W, H = 37, 29
  K = np.array([[41.5, 0., 15.25], [0., 33.75, 17.5], [0., 0., 1.]])            # fx != fy, the principal point off the centre
  pixtocam = np.linalg.inv(K)
  rs = np.random.default_rng(3)
  q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
  q *= np.sign(np.linalg.det(q))
  c2w = np.concatenate([q, np.array([[0.7], [-1.9], [2.3]])], 1)
  px, py = np.meshgrid(np.arange(W), np.arange(H), indexing='xy')
  origins, directions, _, _, _ = ocam.pixels_to_rays(torch.as_tensor(px), torch.as_tensor(py), torch.as_tensor(pixtocam), torch.as_tensor(c2w))
  origins, directions = origins.numpy(), directions.numpy()
  assert origins.dtype == np.float64
  P32 = mesh.world_to_pixel(pixtocam, c2w)
  assert P32.shape == (3, 4) and P32.dtype == np.float32
  assert np.array_equal(P32, mesh.world_to_pixel(torch.as_tensor(pixtocam), torch.as_tensor(c2w)))
  P = P32.astype(np.float64)
  eps, worst = 2. ** -24, 0.
  for t in (0.05, 1., 7.5, 300.):
    X = origins + t * directions
    m = X @ P[:, :3].T + P[:, 3]
    mag = np.abs(X) @ np.abs(P[:, :3]).T + np.abs(P[:, 3])
    u, v, zc = m[..., 0] / m[..., 2], m[..., 1] / m[..., 2], m[..., 2]
    slack = 1e-9 * mag
    bound_u = 1.01 * eps * (mag[..., 0] + (px + 0.5) * mag[..., 2]) / t + (slack[..., 0] + slack[..., 2]) / t
    bound_v = 1.01 * eps * (mag[..., 1] + (py + 0.5) * mag[..., 2]) / t + (slack[..., 1] + slack[..., 2]) / t
    bound_z = eps * mag[..., 2] + slack[..., 2]
    eu, ev, ez = np.abs(u - (px + 0.5)), np.abs(v - (py + 0.5)), np.abs(zc - t)
    print(f't = {t}: max |du| {eu.max():.3e} (bound {bound_u.max():.3e}), |dv| {ev.max():.3e} ({bound_v.max():.3e}), '
          f'|dzc| {ez.max():.3e} ({bound_z.max():.3e})')
    assert (eu <= bound_u).all() and (ev <= bound_v).all() and (ez <= bound_z).all()
    worst = max(worst, eu.max(), ev.max())
  assert worst < 1e-3                                        # far below a pixel: the nearest-pixel lookup is the ray's own pixel
  # the float64 product itself, without the float32 rounding, is exact to float64 accuracy
  K64 = K @ np.diag([1., -1., -1.]) @ np.concatenate([q.T, -(q.T @ c2w[:, 3])[:, None]], 1)
  assert np.array_equal(P32, K64.astype(np.float32))


def test_world_to_pixel_refuses_what_has_no_projection_matrix():
  pixtocam, c2w = np.linalg.inv(T.intrinsics(50., 50., 16., 16.)), T.look_at((2., 1., 1.))
  with pytest.raises(ValueError, match='distortion'):
    mesh.world_to_pixel(pixtocam, c2w, distortion_params=dict(k1=0.1))
  with pytest.raises(ValueError, match='pixtocam_ndc'):
    mesh.world_to_pixel(pixtocam, c2w, pixtocam_ndc=pixtocam)
  with pytest.raises(ValueError, match='FISHEYE'):
    mesh.world_to_pixel(pixtocam, c2w, camtype=camera_utils.ProjectionType.FISHEYE)
  with pytest.raises(ValueError, match='FISHEYE'):
    mesh.world_to_pixel(pixtocam, c2w, camtype='fisheye')
  with pytest.raises(ValueError, match="'pano'"):
    mesh.world_to_pixel(pixtocam, c2w, camtype='pano')
  assert mesh.world_to_pixel(pixtocam, c2w, camtype='perspective').shape == (3, 4)


def test_projection_of_the_restatement_is_world_to_pixel():
  K, c2w = T.intrinsics(13., 17., 8.7, 13.1), T.look_at((2.1, 1.7, 1.3))
  assert np.array_equal(T.projection(K, c2w), mesh.world_to_pixel(np.linalg.inv(K), c2w))


def test_the_restatement_alone_on_the_sphere_scene():
  """The figures of profiles/tsdf_mesh.md: the specification (12 cameras, 33^3, truncation of 3 spacings) gives a closed,
  consistently oriented sphere whatever the kernel does."""
  scene, ref = T.sphere_scene(), T.sphere_reference()
  assert scene['depth'].shape == (12, 96, 96) and ((scene['depth'] > 0) == (scene['acc'] == 1)).all()
  m = ref['mesh']
  stats = mesh.mesh_stats(m['vertices'], m['faces'])
  figures = T.check_sphere_mesh(m['vertices'], m['normals'], m['faces'], stats)
  assert (stats['V'], stats['T'], m['faces_unfiltered'], int((ref['weight'] == 0).sum())) == (5282, 10560, 15864, 1357)
  assert round(figures['max_dev'], 4) == 0.0374 and round(figures['volume_ratio'], 4) == 0.9675
  assert m['colors'].dtype == np.uint8 and m['colors'].shape == m['vertices'].shape
  assert ref['tsdf'].min() >= -1. and ref['tsdf'].max() <= 1. and ref['weight'].max() <= 12


def test_c_entries_validate_their_arguments():
  """Every entry returns MNR_ERR_INVALID_ARGUMENT before a launch (no GPU is touched: the checks come first)."""
  lib = _lib.load()
  bad = _lib.MNR_ERR_INVALID_ARGUMENT
  assert lib.mnr_tsdf_integrate(None, None) == bad
  a = _lib.TsdfArgs()
  assert lib.mnr_tsdf_integrate(C.byref(a), None) == bad and b'volumes' in lib.mnr_last_error()
  buf = (C.c_float * 64)()
  a.tsdf = a.weight = a.proj = a.depth = C.addressof(buf)
  good = dict(nx=2, ny=2, nz=2, spacing=1., trunc=1., F=1, H=2, W=2)
  for change, word in ((dict(nx=0), b'dimension'), (dict(spacing=0.), b'spacing'), (dict(spacing=float('nan')), b'spacing'),
                       (dict(trunc=0.), b'trunc'), (dict(trunc=float('inf')), b'trunc'), (dict(F=-1), b'frames'), (dict(H=0), b'images'),
                       (dict(W=2 ** 24 + 1), b'images'), (dict(origin0=float('inf')), b'origin')):
    for k, v in {**good, 'origin0': 0., **change}.items():
      if k == 'origin0':
        a.origin[0] = v
      else:
        setattr(a, k, v)
    assert lib.mnr_tsdf_integrate(C.byref(a), None) == bad and word in lib.mnr_last_error(), change
  for k, v in good.items():
    setattr(a, k, v)
  a.origin[0] = 0.
  a.rgb = C.addressof(buf)
  assert lib.mnr_tsdf_integrate(C.byref(a), None) == bad and b'both' in lib.mnr_last_error()
  a.rgb, a.color = None, C.addressof(buf)
  assert lib.mnr_tsdf_integrate(C.byref(a), None) == bad and b'both' in lib.mnr_last_error()
  a.color, a.depth = None, None
  assert lib.mnr_tsdf_integrate(C.byref(a), None) == bad and b'proj' in lib.mnr_last_error()
  a.F = 0
  assert lib.mnr_tsdf_integrate(C.byref(a), None) == _lib.MNR_OK          # no frames: a successful no-op, nothing is launched

  m = _lib.MtArgs()
  assert lib.mnr_mt_vertex_valid(None, None, None, None) == bad
  assert lib.mnr_mt_vertex_valid(C.byref(m), None, None, None) == bad and b'mask' in lib.mnr_last_error()
  m.mask = m.base = C.addressof(buf)
  m.nx, m.ny, m.nz = 1, 4, 4
  assert lib.mnr_mt_vertex_valid(C.byref(m), C.addressof(buf), C.addressof(buf), None) == bad and b'dimension' in lib.mnr_last_error()
  m.nx, m.n_verts = 4, 2 ** 31
  assert lib.mnr_mt_vertex_valid(C.byref(m), C.addressof(buf), C.addressof(buf), None) == bad and b'2^31' in lib.mnr_last_error()
  m.n_verts = 1
  assert lib.mnr_mt_vertex_valid(C.byref(m), None, C.addressof(buf), None) == bad and b'valid' in lib.mnr_last_error()
  assert lib.mnr_mt_vertex_valid(C.byref(m), C.addressof(buf), None, None) == bad and b'keep' in lib.mnr_last_error()
  m.n_verts = 0
  assert lib.mnr_mt_vertex_valid(C.byref(m), C.addressof(buf), None, None) == _lib.MNR_OK


def test_entries_lists_and_documents():
  names = _lib.header_symbols()
  for e in ('mnr_tsdf_integrate', 'mnr_mt_vertex_valid'):
    assert e in names and e in _lib._PROTOS and e not in _lib.F32_ABSENT
  f32 = C.CDLL(_lib.LIB_F32_PATH)
  assert hasattr(f32, 'mnr_tsdf_integrate') and hasattr(f32, 'mnr_mt_vertex_valid')
  with open(_lib.HEADER_PATH) as f:
    assert f'#define MNR_TSDF_MAX_FRAMES {_lib.TSDF_MAX_FRAMES}\n' in f.read()
  assert 'tsdf.hip' in build.SOURCES and 'tsdf.hip' in build.SOURCES_F32
  read = lambda rel: open(os.path.join(ROOT, rel)).read()
  for rel, attr in (('hipsim/build.py', 'SOURCES'), ('isa_report.py', 'KERNEL_FILES')):
    assert 'tsdf.hip' in getattr(tool_module(rel), attr), rel
  src = read('multinerf_amd/csrc/tsdf.hip')
  code = src.split('#include')[1]
  assert '#pragma clang fp contract(off)' in code and 'atomic' not in code and 'asm' not in code
  readme = read('README.md')
  assert readme.index('### Extracting a mesh') < readme.index('TSDF fusion') and '--method tsdf' in readme
  assert 'tsdf.hip' in read('DESIGN.md') and os.path.exists(os.path.join(ROOT, 'profiles', 'tsdf_mesh.md'))
  assert os.path.exists(os.path.join(ROOT, 'tools', 'tsdf_probe.py'))


def test_script_command_line():
  import extract_mesh
  args, _ = extract_mesh.parse_args([])
  assert (args.method, args.tsdf_trunc, args.tsdf_split, args.tsdf_stride, args.tsdf_depth, args.acc_threshold) == \
      ('density', 3.0, 'train', 1, 'distance_median', 0.5)
  args, box = extract_mesh.parse_args(['--method', 'tsdf', '--tsdf_trunc', '4.5', '--tsdf_split', 'test', '--tsdf_stride', '3', '--tsdf_depth',
                                       'distance_mean', '--acc_threshold', '0.25', '--bbox', '-2,-2,-2,2,2,2'])
  assert (args.method, args.tsdf_trunc, args.tsdf_split, args.tsdf_stride, args.tsdf_depth, args.acc_threshold) == \
      ('tsdf', 4.5, 'test', 3, 'distance_mean', 0.25) and box == [-2., -2., -2., 2., 2., 2.]
  for bad in (['--method', 'poisson'], ['--tsdf_split', 'val'], ['--tsdf_depth', 'acc']):
    with pytest.raises(SystemExit):
      extract_mesh.parse_args(bad)


def test_tsdf_volume_starts_empty_and_checks_its_arguments():
  v = mesh.TsdfVolume((-1., -1., -1.), (1., 1., 0.), 9, trunc_voxels=2.5, device='cpu')
  assert v.shape == (9, 9, 5) and v.spacing == 0.25 and v.trunc == 0.625 and v.origin == (-1., -1., -1.)
  assert (v.tsdf == 1).all() and (v.weight == 0).all() and (v.color == 0).all() and tuple(v.color.shape) == (9, 9, 5, 3)
  field, valid = v.field()
  assert (field == -1).all() and not valid.any()
  assert mesh.TsdfVolume((-1., -1., -1.), (1., 1., 1.), 5, colors=False, device='cpu').color is None
  with pytest.raises(ValueError, match='trunc_voxels'):
    mesh.TsdfVolume((-1., -1., -1.), (1., 1., 1.), 5, trunc_voxels=0., device='cpu')
  with pytest.raises(ValueError, match='needs rgb'):
    v.integrate(np.ones((4, 4), np.float32), np.zeros((3, 4), np.float32))
  with pytest.raises(ValueError, match='device tensor'):                  # (the HIP path has no CPU fallback)
    v.integrate(np.ones((4, 4), np.float32), np.zeros((3, 4), np.float32), rgb=np.ones((4, 4, 3), np.float32))
