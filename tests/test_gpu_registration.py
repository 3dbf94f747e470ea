"""Mesh registration on the GPU (-m gpu): the kernels of csrc/meshreg.hip through ops.mesh_closest / mesh_face_normals / icp_sums /
crop_polygon and mesh.closest_points / CropVolume / register / geometry_metrics against the NumPy restatement
(tests/registration_ref.py): closest points and normals bit for bit, the sums within the bound of reordering a float64 sum, the crop
mask exactly, the registration against a float64 ICP with brute-force closest points, and eval_mesh.py.  The margins that are
measured (not derived) are recorded in profiles/mesh_registration.md; tests/test_registration_cpu.py holds the restatement's own
known answers."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import geometry_ref as G
from tests import registration_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/mesh_registration.md: max |T P^-1 - I| of mode 'plane' and max |T - T_ref| of mode 'point' after 10 iterations, measured
# on the simulator against the float64 reference; asserted with a factor of 4
PLANE_ERROR = 8.6e-9
POINT_ERROR = 1.2e-8
PERTURBATION = 0.05                                                           # the translation's largest entry; the rotation moves more


def dev(a):
  return torch.from_numpy(np.array(a)).cuda()


def host(t):
  return t.cpu().numpy()


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
  ok = np.array_equal(bits(got), bits(want))
  if not ok:
    bad = np.nonzero((bits(got) != bits(want)).any(-1))[0]
    print(f'{what}: {len(bad)} rows differ; the first: {[(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:5]]}')
  return ok


# ---- closest point

@functools.lru_cache(maxsize=None)
def soup_case():
  verts, faces = G.soup()
  lo, hi = G.soup_box(verts, faces)
  q = G.queries(verts, faces, float(np.float32((hi - lo).max() / 20)))
  return verts, faces, q


def test_closest_point_against_the_restatement():
  verts, faces, q = soup_case()
  v, f, p = dev(verts), dev(faces), dev(q)
  d2, face = ops.point_mesh_distance(p, v, f, check_faces=False)
  x, nrm = ops.mesh_closest(p, face, v, f)
  face_h = host(face)
  assert (face_h[-2:] == -1).all() and (face_h[:-2] >= 0).all()
  want = R.closest(q, face_h, verts, faces)
  assert same(host(x), want[0], 'x') and same(host(nrm), want[1], 'nrm')
  assert np.array_equal(bits(host(x)[-2:]), bits(q[-2:])) and (host(nrm)[-2:] == 0).all()       # face -1: the query itself, no normal
  # every face asked for by hand: the invalid ones (120 .. 123), the degenerate ones (60 .. 62, no normal), ids outside the faces
  ask = np.concatenate([np.arange(len(faces)), [-1, -7, len(faces), 2 ** 31 - 1]]).astype(np.int32)
  pts = q[:len(ask)]
  x, nrm = (host(t) for t in ops.mesh_closest(dev(pts), dev(ask), v, f))
  want = R.closest(pts, ask, verts, faces)
  assert same(x, want[0], 'x by hand') and same(nrm, want[1], 'nrm by hand')
  for k in (120, 121, 122, 123, 304 - 4, 304 - 3, 304 - 2, 304 - 1):
    assert np.array_equal(bits(x[k]), bits(pts[k])) and (nrm[k] == 0).all()
  assert (nrm[[60, 61, 62]] == 0).all() and not np.array_equal(x[60:63], pts[60:63])
  live = np.setdiff1d(np.arange(300), [60, 61, 62, 120, 121, 122, 123])
  assert np.abs(np.linalg.norm(nrm[live].astype(np.float64), axis=1) - 1).max() < 2e-7
  # two runs
  again = ops.mesh_closest(dev(pts), dev(ask), v, f)
  assert np.array_equal(bits(host(again[0])), bits(x)) and np.array_equal(bits(host(again[1])), bits(nrm))


def test_closest_point_is_the_foot_of_the_distance():
  """|p - x|^2 in float64 against the float64 evaluation of the same formula: twice what the float32 restatement deviates, slivers
  (faces 70 .. 119) and the rest apart; and against the d2 that chose the face."""
  verts, faces, q = soup_case()
  v, f = dev(verts), dev(faces)
  live = np.isfinite(q).all(1)
  p = q[live]
  d2, face = ops.point_mesh_distance(dev(p), v, f, check_faces=False)
  x = host(ops.mesh_closest(dev(p), face, v, f)[0]).astype(np.float64)
  face, d2 = host(face), host(d2).astype(np.float64)
  x32, x64 = R.closest(p, face, verts, faces)[0].astype(np.float64), R.closest(p, face, verts, faces, dtype=np.float64)[0]
  pd = p.astype(np.float64)
  dist2 = lambda y: ((pd - y) ** 2).sum(1)
  sliver = (face >= 70) & (face < 120)
  assert sliver.sum() > 20 and (~sliver).sum() > 1000
  for name, sel in (('slivers', sliver), ('the rest', ~sliver)):
    ref = np.abs(dist2(x32) - dist2(x64))[sel].max()
    got = np.abs(dist2(x) - dist2(x64))[sel].max()
    print(f'{name}: |p - x|^2 float32 restatement against float64 {ref:.3e}, the kernel {got:.3e}; against the d2 of the query '
          f'{np.abs(dist2(x) - d2)[sel].max():.3e}')
    assert got <= 2 * ref
  rest = ~sliver
  assert np.abs(dist2(x) - d2)[rest].max() <= 1e-5 * max(d2[rest].max(), 1.)     # forming x in float32: a few 1e-7 of the scene's size


def test_closest_point_of_a_cloud_with_and_without_normals():
  rng = np.random.default_rng(21)
  cloud = rng.uniform(-0.6, 0.6, (2000, 3)).astype(np.float32)
  vn = rng.normal(size=(2000, 3)).astype(np.float32) * rng.uniform(0.1, 10, (2000, 1)).astype(np.float32)
  vn[:50] = 0
  vn[50] = [np.nan, 0, 1]
  vn[51] = [np.inf, 0, 1]
  q = rng.uniform(-0.8, 0.8, (1500, 3)).astype(np.float32)
  q[:60] = cloud[:60] + np.float32(1e-4)                                     # so that the points without a usable normal are found
  faces = np.repeat(np.arange(2000, dtype=np.int32)[:, None], 3, 1)
  c, f, p = dev(cloud), dev(faces), dev(q)
  _, face = ops.point_mesh_distance(p, c, f)
  face_h = host(face)
  assert np.array_equal(face_h[:60], np.arange(60))
  for normals in (None, vn):
    x, nrm = (host(t) for t in ops.mesh_closest(p, face, c, f, vnormals=None if normals is None else dev(normals)))
    want = R.closest(q, face_h, cloud, faces, vnormals=normals)
    assert same(x, want[0], 'x') and same(nrm, want[1], 'nrm')
    assert np.array_equal(bits(x), bits(cloud[face_h] + np.float32(0)))         # the nearest point itself
    if normals is None:
      assert (nrm == 0).all()
    else:
      none = face_h < 52                                                       # the nearest point's normal is 0, NaN or infinite
      assert none[:52].all() and (nrm[none] == 0).all() and np.abs(np.linalg.norm(nrm[~none].astype(np.float64), axis=1) - 1).max() < 2e-7
  got = mesh.closest_points(p, dict(vertices=c, normals=dev(vn)))
  assert same(host(got['normal']), want[1], 'closest_points') and np.array_equal(host(got['face']), face_h)
  assert set(got) == {'point', 'normal', 'distance', 'face'} and (host(mesh.closest_points(p, dict(vertices=c))['normal']) == 0).all()


def test_face_normals_against_the_restatement():
  verts, faces, _ = soup_case()
  got = host(ops.mesh_face_normals(dev(verts), dev(faces)))
  assert same(got, R.face_normals(verts, faces), 'face normals')
  assert (got[[60, 61, 62, 120, 121, 122, 123]] == 0).all() and (got[:60] != 0).any(1).all()
  assert ops.mesh_face_normals(dev(verts), dev(faces[:0])).shape == (0, 3)


# ---- the sums

@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 4099, 65536 + 300])       # one workgroup, its edges, several partials, more than 256 workgroups' worth
def test_icp_sums_against_float64(n):
  rng = np.random.default_rng(100 + n % 1000)
  p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
  x = (p + rng.normal(scale=0.05, size=(n, 3))).astype(np.float32)
  nrm = rng.normal(size=(n, 3))
  nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
  keep = (rng.uniform(size=n) > 1 / 3).astype(np.uint8)
  keep[:1] = 1                                                                 # (n = 1: the one correspondence counts)
  centre = [0.25, -0.125, 0.0625]
  got = host(ops.icp_sums(dev(p), dev(x), dev(nrm), dev(keep), centre))
  terms = R.icp_terms(p, x, nrm, keep, centre)
  want, bound = terms.sum(0), n * 2. ** -52 * np.abs(terms).sum(0)              # the bound of adding n float64 terms in any order
  assert got.shape == (R.ICP_SUMS,) == (ops.L.ICP_SUMS,) and got[0] == keep.sum()
  worst = np.abs(got - want) / np.where(bound > 0, bound, 1.)
  print(f'n = {n}: kept {int(keep.sum())}, the largest error over its bound {worst.max():.3f}')
  assert (np.abs(got - want) <= bound).all(), np.nonzero(np.abs(got - want) > bound)[0]
  again = host(ops.icp_sums(dev(p), dev(x), dev(nrm), dev(keep), centre))
  assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
  if n == 4099:                                                                # and the entries mean what the header says
    S, c = got, np.array(centre)
    k = keep != 0
    pd, xd, nd = p[k].astype(np.float64), x[k].astype(np.float64), nrm[k].astype(np.float64)
    J = np.concatenate([np.cross(pd - c, nd), nd], 1)
    r = ((pd - xd) * nd).sum(1)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = S[20:41]
    assert np.allclose(A, np.triu(J.T @ J), rtol=1e-12, atol=1e-12) and np.allclose(S[41:], J.T @ r, rtol=1e-12, atol=1e-12)
    assert np.allclose(S[7:16].reshape(3, 3), (pd - c).T @ (xd - c), rtol=1e-12) and np.allclose(S[1:4], (pd - c).sum(0), atol=1e-11)
    assert np.isclose(S[18], ((pd - xd) ** 2).sum(), rtol=1e-12) and np.isclose(S[19], (r * r).sum(), rtol=1e-12)


# ---- the crop volume

def crop_points():
  rng = np.random.default_rng(41)
  uni = rng.uniform(-0.8, 0.8, (2000, 3))
  on_v = np.stack([rng.uniform(-0.8, 0.8, 300), rng.choice([-0.5, 0., 0.5], 300), rng.uniform(-0.4, 0.4, 300)], 1)   # on a corner's v
  on_u = np.stack([rng.choice([-0.5, 0., 0.5], 300), rng.uniform(-0.8, 0.8, 300), rng.uniform(-0.4, 0.4, 300)], 1)   # on a corner's u
  corners = np.concatenate([R.l_polygon(), np.zeros((6, 1))], 1)
  ends = np.stack([rng.uniform(-0.5, 0., 200), rng.uniform(-0.5, 0., 200), rng.choice([-0.25, 0.375], 200)], 1)     # on w_min, w_max
  just = np.array([[-0.25, -0.25, np.nextafter(np.float32(-0.25), np.float32(-1))], [-0.25, -0.25, np.nextafter(np.float32(0.375), np.float32(1))]])
  out = np.array([[-0.9, 0, 0], [0.9, -0.25, 0], [0, -0.9, 0], [-0.25, 0.9, 0], [0.25, 0.25, 0], [-0.25, -0.25, -0.9], [-0.25, -0.25, 0.9],
                  [np.nan, 0, 0], [-0.25, np.nan, 0], [-0.25, -0.25, np.nan], [np.inf, -0.25, 0]])
  return np.concatenate([uni, on_v, on_u, corners, ends, just, out]).astype(np.float32)


@pytest.mark.parametrize('axis', ['X', 'Y', 'Z'])
def test_crop_volume_against_the_restatement(axis):
  a = 'XYZ'.index(axis)
  iu, iv, iw = R.UVW[a]
  base = crop_points()                                                         # written for Z: (u, v, w) = (x, y, z)
  pts = np.empty_like(base)
  pts[:, iu], pts[:, iv], pts[:, iw] = base[:, 0], base[:, 1], base[:, 2]
  crop = mesh.CropVolume(R.l_polygon(), axis, -0.25, 0.375)
  got = host(crop.contains(dev(pts)))
  want = R.crop_polygon(pts, R.l_polygon(), a, -0.25, 0.375)
  assert got.dtype == np.bool_ and np.array_equal(got, want), np.nonzero(got != want)[0]
  assert 0.08 < got[:2000].mean() < 0.15                                       # 0.75 of 2.56 in the plane, 0.625 of 1.6 along the axis: 0.114
  tail = got[-11:]
  assert not tail.any() and not got[-13:-11].any() and got[-213:-13].all()      # outside on every side; one ulp past the ends; ON the ends
  xyz = np.zeros((6, 3))
  xyz[:, [iu, iv]] = R.l_polygon()
  xyz[:, iw] = 123.                                                            # (the orthogonal coordinate of an xyz polygon is ignored)
  assert np.array_equal(host(mesh.CropVolume(xyz, a, -0.25, 0.375).contains(dev(pts))), want)
  keep = host(ops.crop_polygon(dev(pts), dev(R.l_polygon()), a, -0.25, 0.375))
  assert keep.dtype == np.uint8 and np.array_equal(keep != 0, want)


def test_crop_volume_refuses_and_reads_json(tmp_path):
  m = ops.L.CROP_MAX_POLYGON
  ang = np.linspace(0, 2 * np.pi, m + 1, endpoint=False)
  big = np.stack([np.cos(ang), np.sin(ang)], 1)
  pts = dev(np.zeros((4, 3), np.float32))
  assert host(mesh.CropVolume(big[:m], 'Z', -1, 1).contains(pts)).all()       # the maximum itself is served
  for bad in (lambda: mesh.CropVolume(big, 'Z', -1, 1), lambda: ops.crop_polygon(pts, dev(big), 2, -1., 1.),
              lambda: ops.crop_polygon(pts, dev(big[:2]), 2, -1., 1.), lambda: ops.crop_polygon(pts, dev(big[:8]), 3, -1., 1.),
              lambda: ops.crop_polygon(pts, dev(big[:8]), 2, 1., -1.), lambda: ops.crop_polygon(pts, dev(big[:8].astype(np.float32)), 2, -1., 1.),
              lambda: mesh.CropVolume(big[:8], 'W', -1, 1), lambda: mesh.CropVolume(big[:8], 'Z', -1, np.nan),
              lambda: mesh.CropVolume(np.full((4, 2), np.inf), 'Z', -1, 1)):
    with pytest.raises(ValueError):
      bad()
  doc = dict(axis_max=0.375, axis_min=-0.25, bounding_polygon=[[x, y, 0.] for x, y in R.l_polygon()], class_name='SelectionPolygonVolume',
             orthogonal_axis='Z', version_major=1, version_minor=0)
  path = tmp_path / 'crop.json'
  path.write_text(json.dumps(doc))
  crop = mesh.CropVolume.from_json(str(path))
  assert crop.axis == 2 and (crop.axis_min, crop.axis_max) == (-0.25, 0.375) and np.array_equal(crop.polygon, R.l_polygon())
  p = crop_points()
  assert np.array_equal(host(crop.contains(dev(p))), R.crop_polygon(p, R.l_polygon(), 2, -0.25, 0.375))
  del doc['axis_min'], doc['orthogonal_axis']
  path.write_text(json.dumps(doc))
  with pytest.raises(ValueError, match='orthogonal_axis, axis_min'):
    mesh.CropVolume.from_json(str(path))


# ---- registration

MAX_DIST = 0.3


@functools.lru_cache(maxsize=None)
def reg_case():
  """(verts, faces, src [1000,3] float32, P): 1000 samples of the test shape moved by the inverse of the perturbation P."""
  verts, faces = R.shape()
  pts = G.sample(verts, faces, np.cumsum(G.face_areas(verts, faces)), 1000, 5)[0]
  P = R.perturbation()
  Pi = np.linalg.inv(P)
  src = (pts.astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
  for a in (verts, faces, src, P):
    a.setflags(write=False)
  return verts, faces, src, P


@functools.lru_cache(maxsize=None)
def reference(mode, iters):
  """The float64 ICP with brute-force closest points, computed once."""
  verts, faces, src, _ = reg_case()
  return R.icp(src, verts, faces, MAX_DIST, mode, iters)


def target():
  verts, faces, _, _ = reg_case()
  return dict(vertices=dev(verts), faces=dev(faces))


def test_register_plane_converges_to_the_pose():
  verts, faces, src, P = reg_case()
  assert verts.shape == (162, 3) and faces.shape == (320, 3)
  timings = {}
  reg = mesh.register(dict(vertices=dev(src)), target(), max_dist=MAX_DIST, mode='plane', max_iters=10, timings=timings)
  T, h = reg['transform'], reg['history']
  err = np.abs(T @ np.linalg.inv(P) - np.eye(4)).max()
  ref_T, ref_h = reference('plane', 6)
  print(f"plane: {reg['iterations']} iterations, max |T P^-1 - I| = {err:.3e} (the float64 reference after 6: "
        f"{np.abs(ref_T @ np.linalg.inv(P) - np.eye(4)).max():.3e}), against the reference {np.abs(T - ref_T).max():.3e}; rmse {[e['inlier_rmse'] for e in h]}")
  assert T.shape == (4, 4) and T.dtype == np.float64 and set(reg) == {'transform', 'fitness', 'inlier_rmse', 'iterations', 'history'}
  assert reg['iterations'] == len(h) - 1 < 10                                  # stopped by its tolerance, not by max_iters
  assert abs(h[-1]['fitness'] - h[-2]['fitness']) < 1e-6 and abs(h[-1]['inlier_rmse'] - h[-2]['inlier_rmse']) < 1e-6
  assert reg['fitness'] == 1. and reg['inlier_rmse'] == h[-1]['inlier_rmse'] < 1e-6
  assert 4 * PLANE_ERROR <= PERTURBATION / 100 and err <= 4 * PLANE_ERROR
  assert abs(h[0]['inlier_rmse'] - ref_h[0][1]) < 1e-6                         # the same start (the steps differ: the rotation is about another centre)
  assert set(timings) == {'move', 'query', 'closest_sums', 'solve'}
  again = mesh.register(dict(vertices=dev(src)), target(), max_dist=MAX_DIST, mode='plane', max_iters=10)
  assert np.array_equal(again['transform'], T)                                 # two runs agree bit for bit
  # from an init, in stages, and a mesh as the source
  moved = (verts.astype(np.float64) @ np.linalg.inv(P)[:3, :3].T + np.linalg.inv(P)[:3, 3]).astype(np.float32)
  half = np.eye(4)
  half[:3, 3] = 0.5 * P[:3, 3]
  st = mesh.register(dict(vertices=dev(moved), faces=dev(faces)), target(), init=half, max_dist=(0.3, 0.1, 0.03), mode='plane', max_iters=10,
                     n_samples=2000, seed=3)
  print('stages:', [(e['stage'], e['iteration'], e['inlier_rmse']) for e in st['history']])
  assert sorted({e['stage'] for e in st['history']}) == [0, 1, 2] and [e['max_dist'] for e in st['history'] if e['iteration'] == 0] == [0.3, 0.1, 0.03]
  assert np.abs(st['transform'] @ np.linalg.inv(P) - np.eye(4)).max() < PERTURBATION / 100 and st['fitness'] == 1.


def test_register_point_descends_like_the_reference():
  verts, faces, src, P = reg_case()
  reg = mesh.register(dict(vertices=dev(src)), target(), max_dist=MAX_DIST, mode='point', max_iters=10, rel_tol=0.)
  ref_T, ref_h = reference('point', 10)
  rmse = [e['inlier_rmse'] for e in reg['history']]
  diff = np.abs(reg['transform'] - ref_T).max()
  print(f'point: rmse {rmse}; after 10 iterations against the reference {diff:.3e}, from the pose '
        f"{np.abs(reg['transform'] @ np.linalg.inv(P) - np.eye(4)).max():.3e}")
  assert reg['iterations'] == 10 and len(rmse) == 11
  assert all(b <= a for a, b in zip(rmse[:-1], rmse[1:])) and rmse[-1] < 0.25 * rmse[0]
  assert diff <= 4 * POINT_ERROR
  print('rmse against the reference', np.abs(np.array(rmse) - np.array([r for _, r in ref_h])).max())
  assert np.abs(np.array(rmse) - np.array([r for _, r in ref_h])).max() <= 4 * POINT_ERROR
  assert abs(np.linalg.det(reg['transform'][:3, :3]) - 1) < 1e-12


def test_register_point_with_scale_moves_toward_the_scale():
  verts, faces, src, P = reg_case()
  small = (src.astype(np.float64) / 1.03).astype(np.float32)
  scale = lambda T: float(np.cbrt(np.linalg.det(T[:3, :3])))
  rigid = mesh.register(dict(vertices=dev(small)), target(), max_dist=MAX_DIST, mode='point', max_iters=10, rel_tol=0.)
  sim = mesh.register(dict(vertices=dev(small)), target(), max_dist=MAX_DIST, mode='point', with_scale=True, max_iters=10, rel_tol=0.)
  print(f"scale: recovered {scale(sim['transform']):.6f} of 1.03; rmse {sim['inlier_rmse']:.3e} against {rigid['inlier_rmse']:.3e} without")
  assert abs(scale(rigid['transform']) - 1) < 1e-12
  assert 1. < scale(sim['transform']) and abs(scale(sim['transform']) - 1.03) < 0.03
  assert sim['inlier_rmse'] < rigid['inlier_rmse']


def test_register_ignores_floaters():
  verts, faces, src, P = reg_case()
  rng = np.random.default_rng(7)
  d = rng.normal(size=(200, 3))
  far = (3. * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)        # 3 from the centre: > 1.8 from a shape inside radius 1.2
  both = np.concatenate([src[:500], far, src[500:]])
  for mode, margin in (('plane', PLANE_ERROR), ('point', POINT_ERROR)):
    kw = dict(max_dist=MAX_DIST, mode=mode, max_iters=10, rel_tol=0. if mode == 'point' else 1e-6)
    clean = mesh.register(dict(vertices=dev(src)), target(), **kw)
    dirty = mesh.register(dict(vertices=dev(both)), target(), **kw)
    print(mode, 'floaters move the transform by', np.abs(clean['transform'] - dirty['transform']).max())
    assert dirty['fitness'] == 1000 / 1200 and clean['fitness'] == 1.
    assert all(e['fitness'] == 1000 / 1200 for e in dirty['history'])
    assert np.abs(clean['transform'] - dirty['transform']).max() <= 4 * margin


def test_register_argument_errors():
  verts, faces, src, P = reg_case()
  s, t = dict(vertices=dev(src)), target()
  cloud = dict(vertices=dev(verts))
  far = dict(vertices=dev(src + np.float32(10)))
  bad = np.eye(4)
  bad[0, 3] = np.nan
  cases = [
      lambda: mesh.register(s, t, max_dist=MAX_DIST, mode='plane', with_scale=True),
      lambda: mesh.register(s, cloud, max_dist=MAX_DIST, mode='plane'),          # a cloud without normals
      lambda: mesh.register(far, t, max_dist=MAX_DIST, mode='plane'),            # no inlier
      lambda: mesh.register(dict(vertices=dev(np.concatenate([src[:5], src[5:] + np.float32(10)]))), t, max_dist=1e-3, init=P, mode='point'),   # 5
      lambda: mesh.register(s, t, max_dist=MAX_DIST, init=bad),
      lambda: mesh.register(s, t, max_dist=MAX_DIST, init=np.eye(3)),
      lambda: mesh.register(s, t, max_dist=MAX_DIST, mode='affine'),
      lambda: mesh.register(s, t, max_dist=(0.3, -0.1)),
      lambda: mesh.register(s, t, max_dist=None),
      lambda: mesh.register(s, t, max_dist=MAX_DIST, crop=mesh.CropVolume(R.l_polygon() + 50., 'Z', -1, 1)),       # nothing inside
      lambda: mesh.geometry_metrics(s, t, n_samples=100, crop=(0, 0, 0, 1, 1, 1)),
  ]
  for n, c in enumerate(cases):
    with pytest.raises(ValueError):
      c()
      print('case', n, 'did not raise')
  vn = np.zeros((len(verts), 3))
  for k in range(3):
    np.add.at(vn, faces[:, k], R.face_normals(verts, faces).astype(np.float64))
  with_normals = dict(vertices=dev(verts), normals=dev(vn.astype(np.float32)))
  ok = mesh.register(s, with_normals, max_dist=MAX_DIST, mode='plane', max_iters=3, rel_tol=0.)       # a cloud WITH normals serves 'plane'
  pose_error = lambda T: np.abs(T @ np.linalg.inv(P) - np.eye(4)).max()
  print('cloud target with normals: pose error', pose_error(np.eye(4)), '->', pose_error(ok['transform']))
  assert ok['iterations'] == 3 and pose_error(ok['transform']) < 0.5 * pose_error(np.eye(4))
  six = mesh.register(dict(vertices=dev(np.concatenate([src[:6], src[6:] + np.float32(10)]))), t, max_dist=1e-3, init=P, mode='point', max_iters=1)
  assert six['history'][0]['fitness'] == 6 / 1000


# ---- geometry_metrics

N_SAMPLES = 6000


def perturbed_mesh():
  verts, faces, _, P = reg_case()
  Pi = np.linalg.inv(P)
  moved = (verts.astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
  return dict(vertices=dev(moved), faces=dev(faces))


def test_metrics_refine():
  _, _, _, P = reg_case()
  t = float(np.linalg.norm(P[:3, 3])) / 5
  key = f'fscore@{t:g}'
  off = mesh.geometry_metrics(perturbed_mesh(), target(), n_samples=N_SAMPLES, thresholds=(t,))
  on = mesh.geometry_metrics(perturbed_mesh(), target(), n_samples=N_SAMPLES, thresholds=(t,), refine=dict(max_dist=MAX_DIST, n_samples=2000))
  print(key, off[key], '->', on[key], 'chamfer', off['chamfer'], '->', on['chamfer'])
  assert off[key] < 0.5 and on[key] > 0.95
  assert 'transform' not in off and all(isinstance(x, float) for x in off.values())
  assert on['transform'].shape == (4, 4) and np.abs(on['transform'] @ np.linalg.inv(P) - np.eye(4)).max() < PERTURBATION / 100
  assert list(on)[:-1] == list(off)
  given = mesh.geometry_metrics(perturbed_mesh(), target(), n_samples=N_SAMPLES, thresholds=(t,), transform=on['transform'])
  assert all(given[k] == on[k] for k in given)                                 # refine only replaces the transform


def test_metrics_crop():
  verts, faces, _, _ = reg_case()
  crop = mesh.CropVolume(R.l_polygon(), 'Z', -0.25, 0.375)
  pred, gt = perturbed_mesh(), target()
  whole = mesh.geometry_metrics(pred, gt, n_samples=N_SAMPLES, thresholds=(0.02,))
  cut = mesh.geometry_metrics(pred, gt, n_samples=N_SAMPLES, thresholds=(0.02,), crop=crop)
  assert whole['n_pred'] == whole['n_gt'] == N_SAMPLES and 0 < cut['n_pred'] < N_SAMPLES and 0 < cut['n_gt'] < N_SAMPLES
  for key, src, dst, seed in (('accuracy', pred, gt, 0), ('completeness', gt, pred, 1)):
    s = mesh.sample_surface(src, N_SAMPLES, seed=seed)['points']
    inside = crop.contains(s)
    d = mesh.point_mesh_distance(s, dst)['distance'][inside].double()            # the distances of the kept samples, to the WHOLE other shape
    assert cut['n_pred' if key == 'accuracy' else 'n_gt'] == int(inside.sum())
    assert cut[key] == float(d.mean()) and cut[f'{key}_median'] == float(d.median())
  assert list(cut) == list(whole)


def test_metrics_normal_consistency():
  verts, faces, _, _ = reg_case()
  plain = mesh.geometry_metrics(target(), target(), n_samples=N_SAMPLES, thresholds=(0.02,))
  r = mesh.geometry_metrics(target(), target(), n_samples=N_SAMPLES, thresholds=(0.02,), normals=True)
  print({k: r[k] for k in r if k.startswith('normal')})
  assert list(r) == list(plain) + ['normal_consistency_acc', 'normal_consistency_comp', 'normal_consistency'] and all(r[k] == plain[k] for k in plain)
  # Float32 rounding shows in two places.  The unit normals and their product: 1e-6.  And the sample's position: one that lies
  # within rounding of an edge (its computed d2 to its own face is noise of (4 u |p|)^2 = 6e-14, so within 2.4e-7 / sin(dihedral)
  # of the edge: about 2e-5 of this shape's area, 0.1 samples of 6000) may find the neighbouring face, whose normal differs by the
  # dihedral angle.  Three such samples are allowed for, each losing at most 1 - (the smallest |n_1 . n_2| over the edges).
  fn = R.face_normals(verts, faces).astype(np.float64)
  edge = {}
  for t, tri in enumerate(faces):
    for k in range(3):
      edge.setdefault(frozenset((int(tri[k]), int(tri[(k + 1) % 3]))), []).append(t)
  assert all(len(ts) == 2 for ts in edge.values())
  cmin = min(abs(fn[a] @ fn[b]) for a, b in edge.values())
  tol = 1e-6 + 3 * (1 - cmin) / N_SAMPLES
  print(f'the smallest |n_1 . n_2| over the edges {cmin:.4f}: tolerance {tol:.3e}')
  assert 0.8 < cmin < 1 and tol < 1e-4
  for k in ('normal_consistency_acc', 'normal_consistency_comp', 'normal_consistency'):
    assert 1 - tol <= r[k] <= 1 + 1e-6
  flipped = dict(vertices=dev(verts), faces=dev(faces[:, ::-1].copy()))
  assert mesh.geometry_metrics(flipped, target(), n_samples=N_SAMPLES, normals=True)['normal_consistency'] >= 1 - tol      # |m . n|: no orientation
  # against a cloud without normals: no keys; with normals: its own
  cloud = dict(vertices=dev(verts))
  assert not any(k.startswith('normal') for k in mesh.geometry_metrics(target(), cloud, n_samples=N_SAMPLES, normals=True))
  unit = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(np.float32)
  with_n = mesh.geometry_metrics(target(), dict(vertices=dev(verts), normals=dev(3 * unit)), n_samples=N_SAMPLES, normals=True)
  assert 0.5 < with_n['normal_consistency'] < 1                                # radial directions are not this shape's normals, but near


# ---- eval_mesh.py

def test_eval_mesh_script_registers(tmp_path):
  """eval_mesh.py --geometry_only with --gt_crop and --icp plane on files written here: the refined transform is written and is the
  pose, and the F-score beats the run without --icp."""
  verts, faces, _, P = reg_case()
  Pi = np.linalg.inv(P)
  moved = (verts.astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32)
  pred, gt, crop, err = (str(tmp_path / n) for n in ('pred.ply', 'gt.ply', 'crop.json', 'error.ply'))
  for path, v in ((pred, moved), (gt, verts)):
    mesh.write_ply(path, dict(vertices=v, normals=(v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), faces=faces))
  big = [[-2., -2., 0.], [2., -2., 0.], [2., 2., 0.], [-2., 2., 0.]]
  with open(crop, 'w') as f:
    json.dump(dict(bounding_polygon=big, orthogonal_axis='Z', axis_min=-0.1, axis_max=2., class_name='SelectionPolygonVolume'), f)
  t = float(np.linalg.norm(P[:3, 3])) / 5
  common = ['--mesh', pred, '--geometry_only', '--gt_mesh', gt, '--gt_crop', crop, '--geometry_samples', '6000', '--geometry_thresholds', f'{t:g}',
            '--geometry_normals']
  scores = {}
  for name, extra in (('plain', []), ('icp', ['--icp', 'plane', '--icp_max_dist', '0.3,0.1', '--icp_iters', '10', '--icp_samples', '2000', '--error_ply', err])):
    out = str(tmp_path / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'eval_mesh.py')] + common + ['--out_dir', out] + extra, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    scores[name] = dict((l.split()[0], float(l.split()[1])) for l in open(os.path.join(out, 'mesh_metric_geometry.txt')).read().splitlines())
    assert ('ICP stage 1 (max_dist 0.1)' in r.stdout and 'ICP seconds: ' in r.stdout) == (name == 'icp')
    assert sorted(os.listdir(out)) == (['mesh_gt_transform_refined.txt'] if name == 'icp' else []) + ['mesh_metric_geometry.txt']
  key = f'fscore@{t:g}'
  assert scores['plain'][key] < 0.5 and scores['icp'][key] > 0.95 and scores['icp']['n_gt'] < 6000       # the crop cuts z < -0.1 away
  assert scores['icp']['normal_consistency'] > scores['plain']['normal_consistency']
  T = np.loadtxt(str(tmp_path / 'icp' / 'mesh_gt_transform_refined.txt'))
  assert T.shape == (4, 4) and np.abs(T @ Pi - np.eye(4)).max() < PERTURBATION / 100
  back = mesh.read_ply(err)
  assert np.array_equal(back['vertices'], moved) and (back['colors'].astype(int).std(0) < 5).all()     # after the ICP every vertex is ON gt: one colour
