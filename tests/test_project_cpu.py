"""The forward camera model, the parts that need no GPU: the NumPy restatement (tests/project_ref.py) against the project's own
ray model (the oracle's pixels_to_rays in float64, the spherical directions restated from mnr_spherical_rays' header), the
fold-back guard's construction and its ValueError, mesh.camera_record's layout and refusals, the C entries' argument checks, and
that the new entries are declared wherever the others are."""

import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from multinerf_amd import _lib, camera_utils, mesh
from oracle import camera_utils as ocam
from tests import project_ref as P
from tests import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 20, 24
TS = (0.3, 1., 4.)
EPS = 2. ** -24

MODELS = {
    'perspective_distorted': dict(camtype='perspective', distortion=P.DISTORTION, K=T.intrinsics(13., 17., 8.7, 13.1)),
    'fisheye': dict(camtype='fisheye', distortion=None, K=T.intrinsics(6.5, 7.5, 9.3, 12.6)),
    'fisheye_distorted': dict(camtype='fisheye', distortion=P.FISHEYE_DISTORTION, K=T.intrinsics(6.5, 7.5, 9.3, 12.6)),
}


def pose():
  rs = np.random.default_rng(3)
  q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
  q *= np.sign(np.linalg.det(q))
  return np.concatenate([q, np.array([[0.7], [-1.9], [2.3]])], 1)


def row_magnitudes(rec, X):
  """mag_r = |M_r0| |x| + |M_r1| |y| + |M_r2| |z| + |M_r3| [..,3]: what one rounding of c_r is relative to."""
  M = np.abs(np.asarray(rec[:12], np.float64).reshape(3, 4))
  return np.abs(X) @ M[:, :3].T + M[:, 3]


@pytest.mark.parametrize('name', list(MODELS))
def test_points_on_the_oracles_rays_project_to_their_pixel(name):
  """origins + t directions of the oracle's float64 rays project to that pixel's index exactly and to s = t, in the float64
  restatement and in the float32 one.

  Tolerance on s.  The oracle's rays end a 10-step Newton iteration in float64; its residual, measured here by distorting the
  undistorted point forward again, is printed (1e-16, far below everything else), so the forward model is the exact inverse up to
  rounding.  The same iteration in float32, the device's, is measured and printed next to it (1e-7 to 2e-7 image-plane units, 1e-6
  pixel).  It is NOT what bounds |s - t|, which is where this test departs from the wording of its issue: a residual moves the ray
  sideways, (u, v) by that many pixels, and leaves s alone (for the perspective model the ray's camera-space z is 1 whatever x and y
  are; for fisheye the direction has unit length whatever theta is).  So s gets the rounding count below, and the residual is held
  against the half pixel that the index has to spare (`du < 1e-3`).  In float32 every c_r is 4 roundings of terms bounded by mag_r plus the record's own rounding (one more): |dc_r| <=
  5 * 2^-24 mag_r.  s = c_2 (perspective) or |c| (fisheye: 3 products, 2 sums and a root on top, |ds| <= sum_r |dc_r| + 3 * 2^-24
  |c|), so |s - t| <= 8 * 2^-24 (mag_0 + mag_1 + mag_2) covers both; float64 gets the same bound with 2^-53 plus the record's float32
  rounding, 2^-24 (mag_0 + mag_1 + mag_2)."""
  m = MODELS[name]
  pixtocam, c2w = np.linalg.inv(m['K']), pose()
  rec = mesh.camera_record(pixtocam, c2w, H, W, distortion_params=m['distortion'], camtype=m['camtype'])
  assert rec.dtype == np.float32 and rec.shape == (_lib.CAM_REC,) and rec[25] == _lib.CAM_MODEL[m['camtype']] and (rec[26], rec[27]) == (H, W)
  px, py = np.meshgrid(np.arange(W), np.arange(H), indexing='xy')
  origins, directions, _, _, _ = ocam.pixels_to_rays(torch.as_tensor(px), torch.as_tensor(py), torch.as_tensor(pixtocam), torch.as_tensor(c2w),
                                                     distortion_params=m['distortion'], camtype=ocam.ProjectionType(m['camtype']))
  origins, directions = origins.numpy(), directions.numpy()
  assert origins.dtype == np.float64
  if m['distortion'] is not None:                           # the Newton iteration's residual: distort(undistort(p)) - p, in pixels
    k = [m['distortion'].get(n, 0.) for n in ('k1', 'k2', 'k3', 'k4', 'p1', 'p2')]
    p = np.stack([px + .5, py + .5, np.ones_like(px, dtype=np.float64)], -1) @ pixtocam.T
    x, y = ocam._radial_and_tangential_undistort(torch.as_tensor(p[..., 0]), torch.as_tensor(p[..., 1]), **m['distortion'])
    bx, by = mesh._distort(x.numpy(), y.numpy(), k)
    print(f'{name}: 10 Newton steps in float64 leave a residual of {max(np.abs(bx - p[..., 0]).max(), np.abs(by - p[..., 1]).max()):.3e}')
    # the same 10 steps in float32, the device's arithmetic (csrc/camera.hip's cam_undistort): what its rays are off by
    p32 = torch.as_tensor(p.astype(np.float32))
    x32, y32 = ocam._radial_and_tangential_undistort(p32[..., 0], p32[..., 1], **m['distortion'])
    assert x32.dtype == torch.float32
    bx, by = mesh._distort(x32.numpy().astype(np.float64), y32.numpy().astype(np.float64), k)
    res32 = max(np.abs(bx - p32[..., 0].numpy()).max(), np.abs(by - p32[..., 1].numpy()).max())
    print(f'{name}: 10 Newton steps in float32 leave a residual of {res32:.3e} image-plane units, {res32 * m["K"][0, 0]:.3e} pixels')
    assert res32 < 16 * EPS * (1. + np.abs(p).max())          # a few ulp of the coordinates: the iteration has converged
  for t in TS:
    X = origins + t * directions
    mag = row_magnitudes(rec, X).sum(-1)
    for dtype, eps in ((np.float64, EPS), (np.float32, 8 * EPS)):
      pr = P.project(rec, X, dtype)
      assert pr['ok'].all() and P.on_image(pr, rec).all()
      assert np.array_equal(pr['u'].astype(np.int64), px) and np.array_equal(pr['v'].astype(np.int64), py)
      du = max(np.abs(pr['u'] - (px + .5)).max(), np.abs(pr['v'] - (py + .5)).max())
      ds, bound = np.abs(pr['s'].astype(np.float64) - t), 1.01 * eps * mag
      print(f'{name} t = {t} {dtype.__name__}: max |uv - centre| {du:.3e} px, max |s - t| {ds.max():.3e} (bound {bound.max():.3e})')
      assert (ds <= bound).all() and du < 1e-3                # the nearest-pixel lookup is the ray's own pixel with room to spare


def test_points_on_the_spherical_rays_project_to_their_pixel():
  """The pano model against mnr_spherical_rays' directions: pixel (h, w) looks along a grid POINT, which the forward model reports
  as (w + 0.5, h + 0.5), half a pixel from every edge.  Row 0 is the pole (every column looks straight up): any column is right
  there, so the column index is checked from row 1 on.  |s - t| as above (directions of unit length)."""
  c2w = pose()
  rec = mesh.camera_record(None, c2w, H, W, camtype='pano')
  assert rec[25] == _lib.CAM_MODEL['pano'] and not rec[12:25].any()
  d = P.spherical_directions(c2w, H, W)
  hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  for t in TS:
    X = c2w[:, 3] + t * d
    mag = row_magnitudes(rec, X).sum(-1)
    for dtype, eps in ((np.float64, EPS), (np.float32, 8 * EPS)):
      pr = P.project(rec, X, dtype)
      assert P.on_image(pr, rec).all()
      assert np.array_equal(pr['v'].astype(np.int64), hh) and np.array_equal(pr['u'].astype(np.int64)[1:], ww[1:])
      ds = np.abs(pr['s'].astype(np.float64) - t)
      print(f'pano t = {t} {dtype.__name__}: max |s - t| {ds.max():.3e} (bound {(1.01 * eps * mag).max():.3e})')
      assert (ds <= 1.01 * eps * mag).all()
  # the seam and the poles: directions just left of column 0 wrap to column 0, straight down goes to the last row
  R, o = c2w[:, :3], c2w[:, 3]
  for local, want in (((1e-4, 0., 1.), (0, H // 2)), ((-1e-4, 0., 1.), (0, H // 2)), ((0., -1., 1e-9), (None, H - 1)), ((0., 1., 1e-9), (None, 0))):
    pr = P.project(rec, o + 2. * (R @ np.array(local)), np.float32)
    assert int(pr['v']) == want[1] and (want[0] is None or int(pr['u']) == want[0]) and 0. <= pr['u'] < W
  # the eye itself has no direction
  at_origin = mesh.camera_record(None, np.eye(3, 4), H, W, camtype='pano')
  assert not P.project(at_origin, np.zeros(3), np.float32)['ok'] and P.project(at_origin, np.array([0., 0., 1e-3]), np.float32)['ok']


def test_fold_back_guard_construction():
  """k1 = -0.3: the radial map r (1 - 0.3 r^2) rises up to r = 1.054 (image radius 0.703) and folds back beyond.  With a focal of
  30 pixels the 24 x 20 image's corners lie at a distorted radius of 0.52: invertible, r2_max is the corner's undistorted squared
  radius times 1.01^2, every pixel lies inside it, and points at undistorted radius 1.1 .. 3 are refused although the polynomial
  sends them INTO the image, mirrored.  With a focal of 15 the corners lie at 1.04, past the fold: ValueError."""
  k = dict(k1=-0.3)
  K = T.intrinsics(30., 30., W / 2., H / 2.)
  pixtocam = np.linalg.inv(K)
  r2 = mesh.fold_back_guard(pixtocam, H, W, [-0.3, 0., 0., 0., 0., 0.])
  rd = math.hypot(W / 2., H / 2.) / 30.
  lo, hi = 0., 1.
  for _ in range(200):                                      # bisection on the rising branch
    mid = 0.5 * (lo + hi)
    lo, hi = (mid, hi) if mid * (1. - 0.3 * mid * mid) < rd else (lo, mid)
  assert abs(r2 - (lo * 1.01) ** 2) < 1e-12 and lo < math.sqrt(1. / 0.9)
  c2w = T.look_at((0., 0., 3.))
  rec = mesh.camera_record(pixtocam, c2w, H, W, distortion_params=k)
  assert rec[24] == np.float32(r2)
  # nothing in the image is dropped: every pixel's corner-to-corner extent comes from inside the guard
  px, py = np.meshgrid(np.arange(W + 1) - 0., np.arange(H + 1) - 0., indexing='xy')
  p = np.stack([px, py, np.ones_like(px)], -1) @ pixtocam.T
  x, y = mesh._undistort(p[..., 0].ravel(), p[..., 1].ravel(), [-0.3, 0., 0., 0., 0., 0.])
  assert (x * x + y * y).max() <= r2 / 1.01 ** 2 + 1e-12
  # the fold: camera-space points at undistorted radius rho, depth 1 (the camera looks down -z of its OpenGL frame, i.e. world -z here)
  R, o = c2w[:, :3], c2w[:, 3]
  rs = np.random.default_rng(5)
  rho, ang = rs.uniform(1.1, 3., 500), rs.uniform(0., 2. * math.pi, 500)
  cam = np.stack([rho * np.cos(ang), -rho * np.sin(ang), -np.ones_like(rho)], -1) * rs.uniform(0.5, 2., (500, 1))
  X = o + cam @ R.T
  for dtype in (np.float64, np.float32):
    pr = P.project(rec, X, dtype)
    assert (pr['s'] > 0).all() and not pr['ok'].any() and not P.on_image(pr, rec).any()
    open_rec = rec.copy()
    open_rec[24] = np.float32(1e30)                         # without the guard a good part of them lands in the image
    assert P.on_image(P.project(open_rec, X, dtype), open_rec).mean() > 0.1
  with pytest.raises(ValueError, match='reaches past'):
    mesh.camera_record(np.linalg.inv(T.intrinsics(15., 15., W / 2., H / 2.)), c2w, H, W, distortion_params=k)
  # fisheye: the radius is the angle and is capped at pi
  assert mesh.fold_back_guard(np.linalg.inv(T.intrinsics(2., 2., W / 2., H / 2.)), H, W, [0.] * 6, fisheye=True) == math.pi ** 2
  wide = mesh.fold_back_guard(np.linalg.inv(T.intrinsics(7., 7., W / 2., H / 2.)), H, W, [0.] * 6, fisheye=True)
  assert abs(wide - (W * W + H * H) / 4. / 49. * 1.01 ** 2) < 1e-12


def test_an_undistorted_record_is_world_to_pixel():
  """Without distortion, a inv-intrinsics times the record's world-to-camera rows IS mesh.world_to_pixel's matrix."""
  K, c2w = T.intrinsics(13., 17., 8.7, 13.1), T.look_at((2.1, 1.7, 1.3))
  rec = mesh.camera_record(np.linalg.inv(K), c2w, H, W).astype(np.float64)
  A = np.concatenate([rec[12:18].reshape(2, 3), [[0., 0., 1.]]], 0)
  assert np.abs(A @ rec[:12].reshape(3, 4) - mesh.world_to_pixel(np.linalg.inv(K), c2w)).max() < 1e-4
  assert not rec[18:24].any() and rec[25] == 0


def test_camera_record_refusals():
  pixtocam, c2w = np.linalg.inv(T.intrinsics(50., 50., 16., 16.)), T.look_at((2., 1., 1.))
  with pytest.raises(ValueError, match='NDC'):
    mesh.camera_record(pixtocam, c2w, 32, 32, pixtocam_ndc=pixtocam)
  projective = pixtocam.copy()
  projective[2] = [1e-6, 0., 1.]
  with pytest.raises(ValueError, match='last row'):
    mesh.camera_record(projective, c2w, 32, 32)
  with pytest.raises(ValueError, match='rotation'):
    mesh.camera_record(pixtocam, c2w * np.array([1.1, 1., 1., 1.]), 32, 32)
  with pytest.raises(ValueError, match='unknown keys'):
    mesh.camera_record(pixtocam, c2w, 32, 32, distortion_params=dict(k5=0.1))
  with pytest.raises(ValueError, match='2\\^24'):
    mesh.camera_record(pixtocam, c2w, 0, 32)
  assert mesh.camera_record(projective, c2w, 32, 32, camtype='pano').shape == (_lib.CAM_REC,)      # (a pano reads no pixtocam)
  for camtype in ('perspective', 'fisheye', camera_utils.ProjectionType.FISHEYE):
    assert mesh.camera_record(pixtocam, c2w, 32, 32, camtype=camtype).shape == (_lib.CAM_REC,)


def test_an_ndc_dataset_is_refused_with_the_reason(monkeypatch):
  """mesh.tsdf_mesh refuses a dataset that renders in an NDC ray space before it touches the model, and says why;
  extract_mesh.py --method tsdf ends with that message."""
  import types
  import extract_mesh
  from multinerf_amd import datasets
  ndc = types.SimpleNamespace(pixtocam_ndc=np.eye(3), distortion_params=None, camtype=camera_utils.ProjectionType.PERSPECTIVE,
                              pixtocams=np.eye(3), size=1, height=4, width=4)
  with pytest.raises(ValueError, match='NDC ray space.*not a world distance'):
    mesh.tsdf_mesh(None, None, ndc, None, (-1., -1., -1.), (1., 1., 1.), 5)
  monkeypatch.setattr(datasets, 'load_dataset', lambda *a, **k: ndc)
  args, box = extract_mesh.parse_args(['--method', 'tsdf', '--resolution', '5'])
  model = types.SimpleNamespace(device='cpu')
  with pytest.raises(SystemExit, match='--method tsdf: .*NDC ray space.*not a world distance'):
    extract_mesh.main_tsdf(args, box, types.SimpleNamespace(data_dir=None), model, types.SimpleNamespace(params=None), 'unused.ply', None)


def test_tsdf_volume_takes_exactly_one_of_proj_and_cameras():
  v = mesh.TsdfVolume((-1., -1., -1.), (1., 1., 1.), 5, colors=False, device='cpu')
  rec = mesh.camera_record(None, T.look_at((2., 1., 1.)), 4, 4, camtype='pano')
  for kw in (dict(), dict(proj=np.zeros((3, 4), np.float32), cameras=rec)):
    with pytest.raises(ValueError, match='exactly one'):
      v.integrate(np.ones((4, 4), np.float32), **kw)
  with pytest.raises(ValueError, match='device tensor'):      # (the HIP path has no CPU fallback)
    v.integrate(np.ones((4, 4), np.float32), cameras=rec)
  assert (v.tsdf == 1).all() and not v.weight.any()


def test_c_entries_validate_their_arguments():
  lib = _lib.load()
  bad = _lib.MNR_ERR_INVALID_ARGUMENT
  assert lib.mnr_tsdf_integrate_cam(None, None) == bad
  a = _lib.TsdfCamArgs()
  assert lib.mnr_tsdf_integrate_cam(C.byref(a), None) == bad and b'volumes' in lib.mnr_last_error()
  buf = (C.c_float * 64)()
  a.tsdf = a.weight = a.cameras = a.depth = C.addressof(buf)
  good = dict(nx=2, ny=2, nz=2, spacing=1., trunc=1., F=1, H=2, W=2, model=0)
  for change, word in ((dict(nx=0), b'dimension'), (dict(spacing=0.), b'spacing'), (dict(trunc=float('inf')), b'trunc'), (dict(F=-1), b'frames'),
                       (dict(H=0), b'images'), (dict(model=3), b'model'), (dict(model=-1), b'model')):
    for k, v in {**good, **change}.items():
      setattr(a, k, v)
    assert lib.mnr_tsdf_integrate_cam(C.byref(a), None) == bad and word in lib.mnr_last_error(), change
  for k, v in good.items():
    setattr(a, k, v)
  a.rgb = C.addressof(buf)
  assert lib.mnr_tsdf_integrate_cam(C.byref(a), None) == bad and b'both' in lib.mnr_last_error()
  a.rgb, a.cameras = None, None
  assert lib.mnr_tsdf_integrate_cam(C.byref(a), None) == bad and b'cameras' in lib.mnr_last_error()
  a.F = 0
  assert lib.mnr_tsdf_integrate_cam(C.byref(a), None) == _lib.MNR_OK            # no frames: a successful no-op, nothing is launched

  rec = (C.c_float * _lib.CAM_REC)()
  rec[25], rec[26], rec[27] = 0., 4., 4.
  assert lib.mnr_project_points(-1, None, rec, None, None, None, None) == bad and b'points' in lib.mnr_last_error()
  assert lib.mnr_project_points(1, None, None, None, None, None, None) == bad and b'record' in lib.mnr_last_error()
  assert lib.mnr_project_points(1, None, rec, None, None, None, None) == bad and b'needs points' in lib.mnr_last_error()
  assert lib.mnr_project_points(0, None, rec, None, None, None, None) == _lib.MNR_OK
  rec[25] = 3.
  assert lib.mnr_project_points(0, None, rec, None, None, None, None) == bad and b'model' in lib.mnr_last_error()
  rec[25], rec[27] = 2., 0.
  assert lib.mnr_project_points(0, None, rec, None, None, None, None) == bad and b'image' in lib.mnr_last_error()


def test_entries_lists_and_documents():
  names = _lib.header_symbols()
  for e in ('mnr_tsdf_integrate_cam', 'mnr_project_points'):
    assert e in names and e in _lib._PROTOS and e not in _lib.F32_ABSENT
  f32 = C.CDLL(_lib.LIB_F32_PATH)
  assert hasattr(f32, 'mnr_tsdf_integrate_cam') and hasattr(f32, 'mnr_project_points')
  read = lambda rel: open(os.path.join(ROOT, rel)).read()
  header = read('include/mnerf.h')
  assert f'#define MNR_CAM_REC {_lib.CAM_REC}\n' in header and P.REC == _lib.CAM_REC
  assert 'MNR_CAM_PERSPECTIVE = 0, MNR_CAM_FISHEYE = 1, MNR_CAM_PANO = 2' in header
  assert _lib.CAM_MODEL == dict(perspective=P.PERSPECTIVE, fisheye=P.FISHEYE, pano=P.PANO)
  # the general kernel keeps the promises of the pinhole one: contraction off, one thread a voxel and nothing shared between them
  section = read('multinerf_amd/csrc/tsdf.hip').split('// ---- any camera model')[1]
  assert 'camera_project.h' in section and 'atomic' not in section and 'asm' not in section
  assert '#pragma clang fp contract(off)' in read('multinerf_amd/csrc/camera_project.h')
  assert 'camera_project.h' in read('DESIGN.md') and os.path.exists(os.path.join(ROOT, 'profiles', 'tsdf_cameras.md'))
  readme = read('README.md')
  assert 'mesh.project_points' in readme and 'camera_record' in readme


def test_probe_command_line():
  from tests.sim_helpers import tool_module
  probe = tool_module('tsdf_probe.py')
  assert probe.parse_args([]).camtype == 'pinhole'
  for camtype in ('pinhole', 'perspective', 'fisheye', 'pano'):
    assert probe.parse_args(['--camtype', camtype, '--frames', '64']).camtype == camtype
  with pytest.raises(SystemExit):
    probe.parse_args(['--camtype', 'ndc'])
