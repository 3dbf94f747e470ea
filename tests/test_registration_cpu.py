"""The NumPy restatement of csrc/meshreg.hip (tests/registration_ref.py) held against answers that are known, and the host side of
the registration that needs no device: the closest point on a triangle in every region, degenerate faces, the meaning of the 47
sums, the crop rule, the test shape, mesh.icp_step against the textbook update, CropVolume's file format, the argument checks
that come before any device work, and eval_mesh.py's flags.  It also prints what profiles/mesh_registration.md records: how far
|p - x|^2 of the float32 restatement lies from its float64 evaluation."""

import importlib.util
import json
import os

import numpy as np
import pytest

from multinerf_amd import _lib as L
from multinerf_amd import mesh
from tests import geometry_ref as G
from tests import registration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_closest_point_in_every_region(dtype):
  verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
  faces = np.array([[0, 1, 2]], np.int32)
  p = np.array([[0.25, 0.25, 1.], [0.25, 0.25, -2.], [2., -1., 0.5], [-1., -1., 0.], [-1., 3., 0.], [0.5, -1., 0.], [1., 1., 3.], [-2., 0.5, 0.],
                [0.25, 0.5, 0.]], np.float32)
  want = np.array([[0.25, 0.25, 0.], [0.25, 0.25, 0.], [1., 0., 0.], [0., 0., 0.], [0., 1., 0.], [0.5, 0., 0.], [0.5, 0.5, 0.], [0., 0.5, 0.],
                   [0.25, 0.5, 0.]])
  x, nrm = R.closest(p, np.zeros(len(p), np.int32), verts, faces, dtype=dtype)
  assert x.dtype == dtype and np.array_equal(x, want) and np.array_equal(nrm, np.broadcast_to([0., 0., 1.], x.shape))
  d2 = G.point_mesh_distance(p, verts, faces, dtype=dtype)[0]
  assert np.array_equal(((p.astype(dtype) - x) ** 2).sum(1), d2)                # exact here: every number is a small dyadic


def test_closest_point_on_degenerate_and_invalid_faces():
  verts = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [5, 5, 5], [np.nan, 0, 0]], np.float32)
  faces = np.array([[3, 3, 3], [0, 1, 2], [0, 0, 1], [0, 1, 4], [0, 1, 7]], np.int32)       # a point, collinear, two equal, NaN, index outside
  p = np.array([[0.5, 1., 0.]] * 7, np.float32)
  x, nrm = R.closest(p, np.array([0, 1, 2, 3, 4, -1, 5], np.int32), verts, faces)
  assert np.array_equal(x[:3], [[5, 5, 5], [0.5, 0, 0], [0.5, 0, 0]]) and np.array_equal(x[3:], p[3:]) and (nrm == 0).all()
  vn = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 3, 4], [0, 0, 0]], np.float32)
  x, nrm = R.closest(p[:2], np.array([0, 1], np.int32), verts, faces, vnormals=vn)
  assert np.array_equal(nrm, np.array([[0, 0.6, 0.8], [0, 0, 0]], np.float32))   # the cloud's point takes its normal, a real face its own (none here)
  q = np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32)
  x, nrm = R.closest(q, np.array([1, 1], np.int32), verts, faces)
  assert np.array_equal(x.view(np.uint32), q.view(np.uint32)) and (nrm == 0).all()


def test_float32_closest_point_against_float64():
  """What profiles/mesh_registration.md records: |p - x|^2 of the float32 restatement against the float64 evaluation of the formula,
  on the soup's queries, slivers (faces 70 .. 119) and the rest apart; and that the foot reproduces the distance that chose the face."""
  verts, faces = G.soup()
  lo, hi = G.soup_box(verts, faces)
  q = G.queries(verts, faces, float(np.float32((hi - lo).max() / 20)))
  q = q[np.isfinite(q).all(1)]
  d2, face = G.point_mesh_distance(q, verts, faces)
  x32, n32 = R.closest(q, face, verts, faces)
  x64, n64 = R.closest(q, face, verts, faces, dtype=np.float64)
  pd = q.astype(np.float64)
  e32, e64 = ((pd - x32.astype(np.float64)) ** 2).sum(1), ((pd - x64) ** 2).sum(1)
  sliver = (face >= 70) & (face < 120)
  near = np.linalg.norm(pd, axis=1) < 2                                        # (six queries lie at distance 50)
  for name, sel in (('slivers', sliver), ('the rest, within the scene', ~sliver & near), ('the rest, at distance 50', ~sliver & ~near)):
    print(f'{name} ({sel.sum()}): |p - x|^2 float32 against float64: {np.abs(e32 - e64)[sel].max():.3e} absolute, '
          f'{(np.abs(e32 - e64) / np.maximum(e64, 1e-30))[sel & (e64 > 1e-6)].max():.3e} relative (d2 > 1e-6); normals {np.abs(n32 - n64)[sel].max():.3e}')
  ok = ~sliver & near
  assert np.abs(e32 - e64)[ok].max() < 1e-6 and np.abs(e32 - d2.astype(np.float64))[ok].max() < 1e-6
  assert np.abs(n32 - n64)[~sliver].max() < 1e-4


def test_the_sums_mean_what_the_header_says():
  assert L.ICP_SUMS == R.ICP_SUMS == 1 + 3 + 3 + 9 + 1 + 1 + 1 + 1 + 21 + 6
  p, x, n = np.array([[1., 2., 3.]], np.float32), np.array([[1., 2., 2.5]], np.float32), np.array([[0., 0., 1.]], np.float32)
  t = R.icp_terms(p, x, n, [1], [1., 1., 1.])[0]
  J = np.array([1., 0., 0., 0., 0., 1.])                                       # (0, 1, 2) x (0, 0, 1) = (1, 0, 0)
  assert t[0] == 1 and np.array_equal(t[1:4], [0, 1, 2]) and np.array_equal(t[4:7], [0, 1, 1.5])
  assert np.array_equal(t[7:16].reshape(3, 3), np.outer([0, 1, 2], [0, 1, 1.5])) and (t[16], t[17], t[18], t[19]) == (5, 3.25, 0.25, 0.25)
  assert np.array_equal(t[20:41], np.outer(J, J)[np.triu_indices(6)]) and np.array_equal(t[41:], J * 0.5)
  assert not R.icp_terms(p, x, n, [0], [1., 1., 1.]).any() and R.icp_terms(p[:0], x[:0], n[:0], [], [0, 0, 0]).shape == (0, 47)


def test_crop_rule_on_the_l_shape():
  poly = R.l_polygon()
  pts = np.array([[-0.25, -0.25, 0], [0.25, -0.25, 0], [-0.25, 0.25, 0], [0.25, 0.25, 0], [0.6, 0, 0], [-0.25, -0.25, 0.375], [-0.25, -0.25, 0.38],
                  [-0.25, -0.25, -0.25], [-0.5, -0.25, 0], [0.5, -0.25, 0], [-0.25, -0.5, 0], [-0.25, 0.5, 0]], np.float32)
  # the three squares of the L, the notch, outside; the ends along the axis count; of the edges, the lower ones (u, v) count
  want = [1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0]
  assert R.crop_polygon(pts, poly, 2, -0.25, 0.375).tolist() == [bool(w) for w in want]
  for axis, (iu, iv, iw) in R.UVW.items():
    moved = np.empty_like(pts)
    moved[:, iu], moved[:, iv], moved[:, iw] = pts[:, 0], pts[:, 1], pts[:, 2]
    assert R.crop_polygon(moved, poly, axis, -0.25, 0.375).tolist() == [bool(w) for w in want]
  assert R.UVW == {0: (1, 2, 0), 1: (0, 2, 1), 2: (0, 1, 2)} and L.CROP_MAX_POLYGON == 4096


def test_the_test_shape():
  verts, faces = R.shape()
  st = mesh.mesh_stats(verts, faces)
  assert (st['V'], st['T'], st['euler'], st['boundary_edges'], st['nonmanifold_edges']) == (162, 320, 2, 0, 0) and st['signed_volume'] > 0
  assert verts.dtype == np.float32 and np.abs(verts).max(0).tolist() == pytest.approx([1., 0.7, 0.5], abs=0.12)
  d = np.linalg.norm(verts / np.float32([1., 0.7, 0.5]), axis=1)
  assert d.min() == pytest.approx(1., abs=1e-3) and d.max() == pytest.approx(1.15, abs=0.01)     # the bump
  P = R.perturbation()
  assert np.allclose(P[:3, :3] @ P[:3, :3].T, np.eye(3), atol=1e-15) and np.isclose(np.trace(P[:3, :3]), 1 + 2 * np.cos(np.deg2rad(5.)))
  assert np.allclose(P[:3, :3] @ [0.3, -0.5, 0.8], [0.3, -0.5, 0.8])


def correspondences():
  verts, faces = R.shape()
  pts = G.sample(verts, faces, np.cumsum(G.face_areas(verts, faces)), 300, 5)[0]
  Pi = np.linalg.inv(R.perturbation())
  p = (pts.astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
  x, n, keep = R.brute_closest(p, verts, faces, 0.3)
  return p, x.astype(np.float32), n.astype(np.float32), keep


def shifted(D, c):
  """The update D, found in coordinates whose origin is c, in the original ones."""
  A, B = np.eye(4), np.eye(4)
  A[:3, 3], B[:3, 3] = c, -np.asarray(c)
  return A @ D @ B


@pytest.mark.parametrize('mode,with_scale', [('point', False), ('point', True), ('plane', False)])
def test_icp_step_is_the_textbook_update(mode, with_scale):
  """mesh.icp_step from the 47 sums against one update of the reference ICP on the same correspondences (taken about the same centre:
  the point-to-plane linearisation depends on where the rotation is taken)."""
  p, x, n, keep = correspondences()
  assert keep.all()
  c = np.array([0.0625, -0.125, 0.03125])
  sums = R.icp_terms(p, x, n, keep, c).sum(0)
  got = mesh.icp_step(sums, c, mode, with_scale)
  pd, xd, nd = (a.astype(np.float64) for a in (p, x, n))
  if mode == 'point':
    mp, mx = pd.mean(0), xd.mean(0)
    U, sv, Vt = np.linalg.svd((pd - mp).T @ (xd - mx))
    Rm = Vt.T @ np.diag([1., 1., np.linalg.det(Vt.T @ U.T)]) @ U.T
    s = sv.sum() / ((pd - mp) ** 2).sum() if with_scale else 1.
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = s * Rm, mx - s * Rm @ mp
    assert np.linalg.det(Rm) == pytest.approx(1.) and (s == 1. or 0.9 < s < 1.1)
  else:
    J = np.concatenate([np.cross(pd - c, nd), nd], 1)
    xi = np.linalg.solve(J.T @ J, -J.T @ (((pd - xd) * nd).sum(1)))
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = R.rodrigues(xi[:3]), xi[3:]
    want = shifted(D, c)
  assert np.abs(got - want).max() < 1e-12
  before = np.sqrt((((pd - xd) * nd).sum(1) ** 2).mean()) if mode == 'plane' else np.sqrt(((pd - xd) ** 2).sum(1).mean())
  q = pd @ got[:3, :3].T + got[:3, 3]
  after = np.sqrt((((q - xd) * nd).sum(1) ** 2).mean()) if mode == 'plane' else np.sqrt(((q - xd) ** 2).sum(1).mean())
  assert after < (0.5 if mode == 'plane' else 1.) * before              # (fixed correspondences: point to surface gains little a step)


def test_the_reference_icp_finds_the_pose():
  """The yardstick itself: point to plane converges to the perturbation within a few iterations, point to surface only descends."""
  verts, faces = R.shape()
  pts = G.sample(verts, faces, np.cumsum(G.face_areas(verts, faces)), 400, 5)[0]
  P = R.perturbation()
  Pi = np.linalg.inv(P)
  src = pts.astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]
  T, h = R.icp(src, verts, faces, 0.3, 'plane', 5)
  # (the samples are float32: they lie within a few 1e-8 of their faces, and that is where the error and the RMSE end)
  assert np.abs(T @ Pi - np.eye(4)).max() < 1e-7 and h[-1][1] < 1e-7 and h[0][1] > 0.03 and all(f == 1 for f, _ in h)
  T, h = R.icp(src, verts, faces, 0.3, 'point', 5)
  assert all(b < a for (_, a), (_, b) in zip(h[:-1], h[1:])) and np.abs(T @ Pi - np.eye(4)).max() > 1e-3


def test_crop_volume_file_format(tmp_path):
  doc = dict(axis_max=4.02, axis_min=-0.5, bounding_polygon=[[x, 7., y] for x, y in R.l_polygon()], class_name='SelectionPolygonVolume',
             orthogonal_axis='Y', version_major=1, version_minor=0)
  path = tmp_path / 'crop.json'
  path.write_text(json.dumps(doc))
  crop = mesh.CropVolume.from_json(str(path))
  assert crop.axis == 1 and (crop.axis_min, crop.axis_max) == (-0.5, 4.02) and np.array_equal(crop.polygon, R.l_polygon())
  for missing in (['axis_max'], ['bounding_polygon', 'orthogonal_axis'], list(doc)):
    path.write_text(json.dumps({k: v for k, v in doc.items() if k not in missing}))
    named = [k for k in ('bounding_polygon', 'orthogonal_axis', 'axis_min', 'axis_max') if k in missing]
    with pytest.raises(ValueError, match=', '.join(named) + '$'):
      mesh.CropVolume.from_json(str(path))
  for bad in (lambda: mesh.CropVolume(R.l_polygon()[:2], 'Z', 0, 1), lambda: mesh.CropVolume(np.zeros((L.CROP_MAX_POLYGON + 1, 2)), 'Z', 0, 1),
              lambda: mesh.CropVolume(R.l_polygon(), 'Q', 0, 1), lambda: mesh.CropVolume(R.l_polygon(), 'Z', 1, 0),
              lambda: mesh.CropVolume(R.l_polygon(), 'Z', 0, float('inf')), lambda: mesh.CropVolume(np.zeros((4, 4)), 'Z', 0, 1)):
    with pytest.raises(ValueError):
      bad()
  assert mesh.CropVolume(R.l_polygon(), 'x', 0, 1).axis == 0 and mesh.CropVolume(R.l_polygon(), 2, 0, 1).axis == 2


def test_register_refuses_before_any_device_work():
  m = dict(vertices=np.zeros((3, 3), np.float32), faces=np.array([[0, 1, 2]], np.int32))
  bad = np.eye(4)
  bad[1, 1] = np.inf
  for kw in (dict(max_dist=0.1, mode='plane', with_scale=True), dict(max_dist=0.1, mode='icp'), dict(max_dist=None), dict(max_dist=0.),
             dict(max_dist=(0.1, float('nan'))), dict(max_dist=()), dict(max_dist=0.1, init=bad), dict(max_dist=0.1, init=np.eye(3)),
             dict(max_dist=0.1, max_iters=-1), dict(max_dist=0.1, n_samples=0)):
    with pytest.raises(ValueError):
      mesh.register(m, m, **kw)


def test_eval_mesh_flags():
  spec = importlib.util.spec_from_file_location('eval_mesh_script', os.path.join(ROOT, 'eval_mesh.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  base = ['--mesh', 'a.ply', '--gt_mesh', 'b.ply']
  a = mod.parse_args(base)
  assert (a.icp, a.gt_crop, a.icp_iters, a.icp_scale, a.icp_samples, a.geometry_normals) == ('none', None, 30, False, 200_000, False)
  a = mod.parse_args(base + ['--icp', 'point', '--icp_max_dist', '0.3,0.1,0.03', '--icp_scale', '--gt_crop', 'c.json', '--geometry_normals'])
  assert a.icp_max_dist == [0.3, 0.1, 0.03] and a.icp_scale and a.gt_crop == 'c.json' and a.geometry_normals
  for bad in (base + ['--icp', 'plane'], base + ['--icp', 'plane', '--icp_max_dist', 'x'], base + ['--icp', 'plane', '--icp_max_dist', '0.1', '--icp_scale'],
              ['--mesh', 'a.ply', '--gt_crop', 'c.json'], ['--mesh', 'a.ply', '--icp', 'point', '--icp_max_dist', '0.1'], base + ['--icp', 'affine']):
    with pytest.raises(SystemExit):
      mod.parse_args(bad)
