"""World point -> pixel on the GPU (-m gpu): mnr_project_points through ops.project_points against the NumPy restatement
(tests/project_ref.py), the round trip through the project's own ray generators on the device, the fold-back guard, and the
wrappers' refusals."""

import functools
import math

import numpy as np
import pytest
import torch

from multinerf_amd import _lib, camera_utils, mesh, ops
from tests import project_ref as P
from tests import tsdf_ref as T

pytestmark = pytest.mark.gpu

H, W = P.H, P.W
N_POINTS = 4096
TS = (0.3, 1., 4.)
EPS = 2. ** -24


def dev(a, dtype=np.float32):
  return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def records(model):
  """[3] records around tests/project_ref.poses(): one camera outside the box, one inside it, one that sees about half of it."""
  if model == 'pano':
    return tuple(P.record(None, c, 'pano') for c in P.poses())
  if model == 'fisheye':
    return tuple(P.record(K, c, 'fisheye', P.FISHEYE_DISTORTION) for K, c in zip(P.fisheye_intrinsics(), P.poses()))
  return tuple(P.record(K, c, 'perspective', P.DISTORTION) for K, c in zip(P.intrinsics(), P.poses()))


@functools.lru_cache(maxsize=None)
def points(model):
  pts = np.random.default_rng({'perspective': 1, 'fisheye': 2, 'pano': 3}[model]).uniform(-1.2, 1.2, (N_POINTS, 3)).astype(np.float32)
  pts.setflags(write=False)
  return pts


@pytest.mark.parametrize('model', ['perspective', 'fisheye', 'pano'])
def test_leaf_against_the_float64_restatement(model):
  """valid agrees except where the float64 (u, v) is within delta of a pixel edge or of the guard; uv and s agree within delta.
  delta is four times the float32 restatement's own worst deviation from float64 on these points (the device's atan2f and acosf
  are within a few ulp, not correctly rounded), per quantity: pixels, world units, the guard's units."""
  pts = points(model)
  compared = 0
  for n, rec in enumerate(records(model)):
    dv = P.deviation(rec, pts)
    delta = {k: 4. * v for k, v in dv.items()}
    print(f'{model} camera {n}: delta uv {delta["uv"]:.3e} px, s {delta["s"]:.3e}, guard {delta["lhs"]:.3e}')
    assert 0. < delta['uv'] < 1e-2 and 0. < delta['s'] < 1e-4
    want = P.project(rec, pts, np.float64)
    want_valid = P.on_image(want, rec)
    uv, s, valid = (t.cpu().numpy() for t in ops.project_points(dev(pts), rec))
    assert uv.shape == (N_POINTS, 2) and s.shape == (N_POINTS,) and valid.dtype == bool
    decided = ~P.undecided(want, rec, delta)
    assert decided.mean() > 0.99 and want_valid.mean() > 0.05
    assert np.array_equal(valid[decided], want_valid[decided])
    m = decided & want_valid
    du, dvv = np.abs(uv[m, 0] - want['u'][m]), np.abs(uv[m, 1] - want['v'][m])
    if model == 'pano':
      du = np.minimum(du, np.abs(W - du))                   # (the seam: u = 0 and u = W name one direction)
    ds = np.abs(s[m] - want['s'][m])
    print(f'{model} camera {n}: {int(m.sum())} valid points, max |du| {du.max():.3e}, |dv| {dvv.max():.3e}, |ds| {ds.max():.3e}')
    assert du.max() <= delta['uv'] and dvv.max() <= delta['uv'] and ds.max() <= delta['s']
    compared += int(m.sum())
    if model == 'perspective':                              # + - x / only: the float32 restatement bit for bit, u, v and s whatever valid is
      same = P.project(rec, pts, np.float32)
      for name, got in (('u', uv[:, 0]), ('v', uv[:, 1]), ('s', s)):
        np.testing.assert_array_equal(got, same[name], err_msg=name)      # (equal values, a NaN equal to a NaN)
      assert np.array_equal(valid, P.on_image(same, rec))
  assert compared > N_POINTS // 2


def rays_of(model, rec_pose, K, distortion):
  """(origins, directions) [H,W,3] float32 on the device from the project's own generators."""
  c2w = dev(rec_pose)
  if model == 'pano':
    return ops.spherical_rays(c2w, H, W)[:2]
  ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.int32).cuda(), torch.arange(W, dtype=torch.int32).cuda(), indexing='ij')
  return camera_utils.pixels_to_rays(xs, ys, dev(np.linalg.inv(K)), c2w, distortion_params=distortion,
                                     camtype=camera_utils.ProjectionType(model))[:2]


@pytest.mark.parametrize('model,distortion', [('perspective', P.DISTORTION), ('fisheye', None), ('fisheye', P.FISHEYE_DISTORTION), ('pano', None)],
                         ids=['perspective_distorted', 'fisheye', 'fisheye_distorted', 'pano'])
def test_round_trip_on_the_device(model, distortion):
  """origins + t directions of the device's own rays project back to their pixel, exactly: a pixel's own ray is half a pixel from
  every edge (the device's 10 float32 Newton steps leave a residual of 1e-6 of that), so there is no boundary case.  Row 0 of a
  panorama is the pole, where every column is the same direction: its column index is not checked.

  s against t.  All float32: the ray's direction (3 products, 2 sums, and sinf / cosf for a fisheye lens), the point o + t d
  (2 roundings), the record (1), c_r (4), |c| (3 more): under 20 roundings, each at most 2^-24 of mag = sum_r (|M_r0| |x| + |M_r1| |y| +
  |M_r2| |z| + |M_r3|).  Bound: 24 * 2^-24 mag."""
  pose = P.poses()[0]
  K = None if model == 'pano' else (P.fisheye_intrinsics() if model == 'fisheye' else P.intrinsics())[0]
  rec = P.record(K, pose, model, distortion)
  origins, directions = rays_of(model, pose, K, distortion)
  hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  M = np.abs(rec[:12].astype(np.float64).reshape(3, 4))
  for t in TS:
    X = (origins + t * directions).reshape(-1, 3).contiguous()
    uv, s, valid = (a.cpu().numpy() for a in ops.project_points(X, rec))
    assert valid.all()
    pu, pv = uv[:, 0].astype(np.int64).reshape(H, W), uv[:, 1].astype(np.int64).reshape(H, W)
    first = 1 if model == 'pano' else 0
    assert np.array_equal(pv, hh) and np.array_equal(pu[first:], ww[first:])
    mag = (np.abs(X.cpu().numpy().astype(np.float64)) @ M[:, :3].T + M[:, 3]).sum(-1)
    ds = np.abs(s.astype(np.float64) - t)
    print(f'{model} t = {t}: max |s - t| {ds.max():.3e} (bound {(24 * EPS * mag).max():.3e}), max |uv - centre| '
          f'{np.abs(uv - np.floor(uv) - 0.5)[W * first:].max():.3e} px')
    assert (ds <= 24 * EPS * mag).all()


def fold_back_camera():
  """k1 = -0.3 at a focal of 30 pixels: the 24 x 20 image ends at a distorted radius of 0.52, the fold is at 0.70."""
  c2w = T.look_at((0., 0., 3.))
  return P.record(T.intrinsics(30., 30., W / 2., H / 2.), c2w, 'perspective', dict(k1=-0.3)), c2w


def test_fold_back_points_are_not_valid():
  """Points in front of the camera at an undistorted radius of 1.1 .. 3 are sent INTO the image by the polynomial, mirrored (a good
  part of them: checked with the guard opened); none is valid."""
  rec, c2w = fold_back_camera()
  rs = np.random.default_rng(5)
  rho, ang = rs.uniform(1.1, 3., N_POINTS), rs.uniform(0., 2. * math.pi, N_POINTS)
  cam = np.stack([rho * np.cos(ang), -rho * np.sin(ang), -np.ones_like(rho)], -1) * rs.uniform(0.5, 2., (N_POINTS, 1))
  X = dev(c2w[:, 3] + cam @ c2w[:, :3].T)
  uv, s, valid = ops.project_points(X, rec)
  assert not valid.any() and (s > 0).all()
  on_image = (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
  assert on_image.float().mean() > 0.1                      # (uv is written whatever valid is: the mirrored landing is visible)
  opened = rec.copy()
  opened[24] = np.float32(1e30)
  assert ops.project_points(X, opened)[2].float().mean() > 0.1
  # and points inside the image's own cone stay valid
  near_axis = dev(c2w[:, 3] + (np.stack([0.3 * np.cos(ang), -0.3 * np.sin(ang), -np.ones_like(rho)], -1) * 2.) @ c2w[:, :3].T)
  assert ops.project_points(near_axis, rec)[2].all()


def test_mesh_project_points_and_shapes():
  """mesh.project_points builds the record itself, keeps the leading shape and takes host arrays."""
  K, c2w = P.fisheye_intrinsics()[0], P.poses()[0]
  pts = points('fisheye').reshape(64, 64, 3)
  uv, s, valid = mesh.project_points(pts, np.linalg.inv(K), c2w, H, W, distortion_params=P.FISHEYE_DISTORTION, camtype='fisheye')
  assert tuple(uv.shape) == (64, 64, 2) and tuple(s.shape) == (64, 64) and valid.dtype == torch.bool
  ref = ops.project_points(dev(pts.reshape(-1, 3)), P.record(K, c2w, 'fisheye', P.FISHEYE_DISTORTION))
  assert torch.equal(uv.reshape(-1, 2), ref[0]) and torch.equal(s.reshape(-1), ref[1]) and torch.equal(valid.reshape(-1), ref[2])
  empty = ops.project_points(torch.zeros((0, 3), device='cuda'), records('pano')[0])
  assert tuple(empty[0].shape) == (0, 2) and tuple(empty[2].shape) == (0,)


def test_refusals():
  pts = dev(points('pano'))
  rec = records('perspective')[0]
  with pytest.raises(ValueError, match=r'\[28\]'):
    ops.project_points(pts, rec[:27])
  with pytest.raises(ValueError, match='one camera model'):
    ops.project_points(pts, np.concatenate([rec[:25], [7.], rec[26:]]).astype(np.float32))
  with pytest.raises(ValueError, match='not finite'):
    ops.project_points(pts, np.concatenate([rec[:3], [np.nan], rec[4:]]).astype(np.float32))
  with pytest.raises(ValueError, match=r'\[N,3\]'):
    ops.project_points(pts[:, :2].contiguous(), rec)
  pixtocam, c2w = np.linalg.inv(P.intrinsics()[0]), P.poses()[0]
  with pytest.raises(ValueError, match='NDC'):
    mesh.camera_record(pixtocam, c2w, H, W, pixtocam_ndc=pixtocam)
  projective = pixtocam.copy()
  projective[2, 0] = 1e-4
  with pytest.raises(ValueError, match='last row'):
    mesh.project_points(pts, projective, c2w, H, W)
  assert _lib.CAM_REC == 28
