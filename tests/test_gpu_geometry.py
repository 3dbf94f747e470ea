"""Mesh geometry on the GPU (-m gpu): the kernels of csrc/meshdist.hip through ops.point_mesh_distance / mesh_grid_build / mesh_sample and
mesh.sample_surface / point_mesh_distance / geometry_metrics against the NumPy restatement (tests/geometry_ref.py, every query against
every face) bit for bit, on every grid; the sampler bit for bit and its statistics; a point cloud against scipy's cKDTree; the
analytic sphere; the metrics on shapes whose answers are known; argument checks, degenerate inputs and eval_mesh.py.
tests/test_geometry_cpu.py holds the restatement's own known answers."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import geometry_ref as G
from tests import raster_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE_D2 = np.float32(np.inf).view(np.uint32)


def dev(a):
  return torch.from_numpy(np.array(a)).cuda()


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(points, verts, faces, **kw):
  kw.setdefault('check_faces', False)
  out = ops.point_mesh_distance(dev(points), dev(verts), dev(faces), **kw)
  assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and tuple(out[0].shape) == tuple(out[1].shape) == (len(points),)
  return tuple(o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def case(flat):
  """(verts, faces, queries, the cell that is a twentieth of the box) of the soup, or of the soup flattened to z = 0."""
  verts, faces = G.soup(flat=flat)
  lo, hi = G.soup_box(verts, faces)
  cell = float(np.float32((hi - lo).max() / 20))
  q = G.queries(verts, faces, cell)
  for a in (verts, faces, q):
    a.setflags(write=False)
  return verts, faces, q, cell


@functools.lru_cache(maxsize=None)
def restated(flat, max_dist=None, dtype=np.float32):
  """The brute-force restatement, computed once and shared."""
  verts, faces, q, _ = case(flat)
  out = G.point_mesh_distance(q, verts, faces, max_dist=max_dist, dtype=dtype)
  for a in out:
    a.setflags(write=False)
  return out


def same(got, want):
  ok = np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
  if not ok:
    bad = np.nonzero((bits(got[0]) != bits(want[0])) | (got[1] != want[1]))[0]
    print(f'{len(bad)} queries differ; the first: {[(int(i), float(got[0][i]), int(got[1][i]), float(want[0][i]), int(want[1][i])) for i in bad[:5]]}')
  return ok


# ---- against the restatement, on every grid

@pytest.mark.parametrize('flat', [False, True], ids=['soup', 'flat'])
def test_distance_against_the_restatement_on_every_grid(flat):
  verts, faces, q, twentieth = case(flat)
  want = restated(flat)
  assert (want[1][np.isfinite(q).all(1)] >= 0).all() and (want[1][-2:] == -1).all() and (bits(want[0][-2:]) == NONE_D2).all()
  assert not np.isin(want[1], [120, 121, 122, 123]).any() and not np.isin(want[1], np.arange(50, 60)).any()   # invalid; the lower id wins
  grids = {}
  for name, cell in (('auto', None), ('single', 10.), ('twentieth', twentieth)):
    grids[name] = ops.mesh_grid_build(dev(verts), dev(faces), cell=cell)
    got = run(q, verts, faces, grid=grids[name], return_shells=True)
    print(name, 'dims', grids[name]['dims'], 'pairs per face', grids[name]['pairs'] / grids[name]['n_valid'], 'mean shells', got[2].mean())
    assert same(got, want), name
  assert grids['single']['dims'] == [1, 1, 1] and grids['single']['pairs'] == grids['single']['n_valid'] == 296
  assert max(grids['twentieth']['dims']) in (20, 21) and min(grids['twentieth']['dims']) == (1 if flat else max(grids['twentieth']['dims']))
  assert flat == (grids['auto']['dims'][2] == 1) and grids['auto']['pairs'] <= ops.MESH_GRID_PAIRS_PER_FACE * 296
  assert same(run(q, verts, faces), want) and same(run(q, verts, faces, cell=twentieth), want)       # two runs; grid built inside
  # against float64: four times what the float32 restatement deviates from the float64 one on these inputs
  live = np.isfinite(q).all(1)
  d32, d64 = np.sqrt(want[0][live].astype(np.float64)), np.sqrt(restated(flat, dtype=np.float64)[0][live])
  tol = 4 * np.abs(d32 - d64).max()
  got = np.sqrt(run(q, verts, faces)[0][live].astype(np.float64))
  print(f'float32 restatement against float64: {tol / 4:.3e} in distance; the kernel: {np.abs(got - d64).max():.3e}')
  assert np.abs(got - d64).max() <= tol


def test_the_pair_list_is_deterministic():
  verts, faces, _, twentieth = case(False)
  a, b = (ops.mesh_grid_build(dev(verts), dev(faces), cell=twentieth) for _ in range(2))
  assert torch.equal(a['cell_start'], b['cell_start']) and torch.equal(a['pair_faces'], b['pair_faces'])
  start, pf = a['cell_start'].cpu().numpy(), a['pair_faces'].cpu().numpy()
  assert start[0] == 0 and start[-1] == len(pf) == a['pairs'] and (np.diff(start) >= 0).all()
  for c in np.nonzero(np.diff(start) > 1)[0][:50]:
    assert (np.diff(pf[start[c]:start[c + 1]]) > 0).all()                     # a cell's faces ascending, each once
  assert (np.bincount(pf, minlength=len(faces))[[120, 121, 122, 123]] == 0).all()
  assert np.bincount(pf, minlength=len(faces))[124] > 1000                  # the face that spans the box


def test_sparse_clusters_walk_empty_shells():
  verts, faces, q, cell = G.sparse_case()
  want = G.point_mesh_distance(q, verts, faces)
  got = run(q, verts, faces, cell=cell, return_shells=True)
  assert same(got, want)
  assert got[2].max() >= 40 and ops.mesh_grid_build(dev(verts), dev(faces), cell=cell)['dims'][0] >= 100
  assert same(run(q, verts, faces), want)


def test_max_dist():
  verts, faces, q, twentieth = case(False)
  q = q[:1000]
  d = np.sqrt(restated(False)[0][:1000].astype(np.float64))
  for max_dist in (0.5 * d.min(), 0.05, 0.3):
    want = G.point_mesh_distance(q, verts, faces, max_dist=max_dist)
    assert same(run(q, verts, faces, max_dist=max_dist), want) and same(run(q, verts, faces, max_dist=max_dist, cell=twentieth), want)
    print(max_dist, 'found', int((want[1] >= 0).sum()))
    assert (want[1] >= 0).sum() == (0 if max_dist < d.min() else (want[0] <= np.float32(max_dist) ** 2).sum())
  assert 0 < (G.point_mesh_distance(q, verts, faces, max_dist=0.05)[1] >= 0).sum() < 1000       # 0.05 cuts the set


def test_point_cloud_against_ckdtree():
  from scipy.spatial import cKDTree
  rng = np.random.default_rng(21)
  cloud = rng.uniform(-0.6, 0.6, (2000, 3)).astype(np.float32)
  q = rng.uniform(-0.8, 0.8, (1500, 3)).astype(np.float32)
  faces = np.repeat(np.arange(2000, dtype=np.int32)[:, None], 3, 1)
  want32, want64 = G.point_mesh_distance(q, cloud, faces), G.point_mesh_distance(q, cloud, faces, dtype=np.float64)
  got = run(q, cloud, faces)
  assert same(got, want32)
  dist, idx = cKDTree(cloud.astype(np.float64)).query(q.astype(np.float64))
  tol_d2 = 4 * np.abs(want32[0].astype(np.float64) - want64[0]).max()
  tol_d = 4 * np.abs(np.sqrt(want32[0].astype(np.float64)) - np.sqrt(want64[0])).max()
  print(f'cloud: float32 against float64 {tol_d2 / 4:.3e} in d2, {tol_d / 4:.3e} in distance; against cKDTree '
        f'{np.abs(got[0] - dist ** 2).max():.3e} and {np.abs(np.sqrt(got[0].astype(np.float64)) - dist).max():.3e}')
  assert np.abs(got[0].astype(np.float64) - dist ** 2).max() <= tol_d2
  assert np.abs(np.sqrt(got[0].astype(np.float64)) - dist).max() <= tol_d
  m = mesh.point_mesh_distance(dev(q), dict(vertices=dev(cloud)))               # a dict without faces is a cloud
  ulps = np.abs(bits(m['distance'].cpu().numpy()).astype(np.int64) - bits(np.sqrt(want32[0])).astype(np.int64))
  assert ulps.max() <= 1 and np.array_equal(m['face'].cpu().numpy(), want32[1])     # (torch's sqrt is not part of the contract: one ulp)


def test_degenerate_inputs():
  verts, faces, q, _ = case(False)
  nothing = lambda out, n: len(out[0]) == n and (bits(out[0]) == NONE_D2).all() and (out[1] == -1).all()
  assert nothing(run(q[:0], verts, faces), 0)
  assert nothing(run(q, verts, faces[:0]), 1500)
  assert nothing(run(q, verts, faces[120:124]), 1500)                          # every face invalid
  assert nothing(run(q, verts[:0], faces), 1500)
  g = ops.mesh_grid_build(dev(verts), dev(faces[120:124]))
  assert g['n_valid'] == 0 and g['pairs'] == 0 and g['dims'] == [1, 1, 1] and g['pair_faces'].shape[0] == 0
  one = np.array([[0, 0, 0]], np.int32)                                        # one point: the box has no extent
  got = run(q[:64], verts, one)
  assert same(got, G.point_mesh_distance(q[:64], verts, one))


def test_argument_checks():
  verts, faces, q, _ = case(False)
  v, f, p = dev(verts), dev(faces[:40].copy()), dev(q)
  ok = ops.point_mesh_distance(p, v, f)
  grid = ops.mesh_grid_build(v, f)
  cases = [
      lambda: ops.point_mesh_distance(p.double(), v, f),
      lambda: ops.point_mesh_distance(p[:, :2], v, f),
      lambda: ops.point_mesh_distance(p, v.double(), f),
      lambda: ops.point_mesh_distance(p, v, f.long()),
      lambda: ops.point_mesh_distance(p, v, f.reshape(-1, 2)),
      lambda: ops.point_mesh_distance(p, v, dev(faces)),                      # indices -1 and V, checked
      lambda: ops.point_mesh_distance(p, v, f, max_dist=0.),
      lambda: ops.point_mesh_distance(p, v, f, max_dist=-1.),
      lambda: ops.point_mesh_distance(p, v, f, max_dist=float('inf')),
      lambda: ops.point_mesh_distance(p, v, f, max_dist=float('nan')),
      lambda: ops.point_mesh_distance(p, v, f, cell=0.),
      lambda: ops.point_mesh_distance(p, v, f, cell=float('nan')),
      lambda: ops.point_mesh_distance(p, v, f, cell=1e-5),                    # more than 1024 cells an axis
      lambda: ops.point_mesh_distance(p, v, f, grid=grid, cell=0.1),
      lambda: ops.point_mesh_distance(p, v, f, grid=dict(grid, dims=[1, 1, 1])),
      lambda: ops.point_mesh_distance(p, v, f, grid=dict(grid, cell_start=grid['cell_start'].int())),
      lambda: ops.point_mesh_distance(p.t().contiguous().t(), v, f),
      lambda: ops.mesh_sample(v, f, torch.cumsum(ops.mesh_face_areas(v, f), 0).float(), 10, 0),
      lambda: ops.mesh_sample(v, f, torch.cumsum(ops.mesh_face_areas(v, f), 0)[:-1], 10, 0),
      lambda: ops.mesh_sample(v, f, torch.cumsum(ops.mesh_face_areas(v, f), 0), -1, 0),
      lambda: ops.mesh_sample(v, f, torch.cumsum(ops.mesh_face_areas(v, f), 0), 10, -1),
      lambda: ops.mesh_sample(v, f, torch.zeros((40,), dtype=torch.float64).cuda(), 10, 0),      # no area
      lambda: mesh.geometry_metrics(dict(vertices=v, faces=f), dict(vertices=v, faces=f), n_samples=100, max_dist=0.),
      lambda: mesh.geometry_metrics(dict(vertices=v, faces=f), dict(vertices=v, faces=f), n_samples=100, thresholds=(0.1, -1.)),
      lambda: mesh.geometry_metrics(dict(vertices=v, faces=f), dict(vertices=v, faces=f), n_samples=100, transform=np.eye(3)),
      lambda: mesh.geometry_metrics(dict(vertices=v, faces=f), dict(vertices=v, faces=f), n_samples=100, bbox=(0, 0, 0, 1, 1)),
      lambda: mesh.geometry_metrics(dict(vertices=v, faces=f), dict(vertices=v, faces=f), n_samples=100, bbox=(5, 5, 5, 6, 6, 6)),
  ]
  if os.environ.get('MNR_TESTS_ON_SIMULATOR') != '1':       # (on the simulator every tensor is a host tensor)
    cases.append(lambda: ops.point_mesh_distance(p.cpu(), v, f))
  for n, c in enumerate(cases):
    with pytest.raises(ValueError):
      c()
      print('case', n, 'did not raise')
  again = ops.point_mesh_distance(p, v, f)
  assert torch.equal(again[0], ok[0]) and torch.equal(again[1], ok[1])        # and nothing was disturbed


# ---- sampling

def small_mesh():
  """Two triangles of area 1 and 3, one without area (collinear corners) and one with an index outside the vertices."""
  verts = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1], [1, 1, 1], [2, 2, 2], [3, 3, 3]], np.float32)
  faces = np.array([[0, 1, 2], [6, 7, 8], [3, 4, 5], [0, 1, 9]], np.int32)
  return verts, faces


def test_sampling_against_the_restatement():
  verts, faces, _, _ = case(False)
  v, f = dev(verts), dev(faces)
  area = ops.mesh_face_areas(v, f)
  want_area = G.face_areas(verts, faces)
  assert np.array_equal(area.cpu().numpy(), want_area) and (want_area[[60, 61, 62, 120, 121, 122, 123]] == 0).all()
  cum = torch.cumsum(area, 0)
  T = len(faces)
  assert np.abs(cum.cpu().numpy() - np.cumsum(want_area)).max() <= T * 2. ** -53 * np.cumsum(want_area)[-1]
  for n, seed in ((1001, 0), (257, 123456789)):
    pts, face = ops.mesh_sample(v, f, cum, n, seed)
    want = G.sample(verts, faces, cum.cpu().numpy(), n, seed)
    assert np.array_equal(face.cpu().numpy(), want[1]) and np.array_equal(bits(pts.cpu().numpy()), bits(want[0]))
    assert (want_area[want[1]] > 0).all()
  assert ops.mesh_sample(v, f, cum, 0, 0)[0].shape == (0, 3)
  a, b = mesh.sample_surface(dict(vertices=v, faces=f), 500, seed=3), mesh.sample_surface(dict(vertices=v, faces=f), 500, seed=3)
  assert torch.equal(a['points'], b['points']) and torch.equal(a['face'], b['face'])
  assert not torch.equal(a['points'], mesh.sample_surface(dict(vertices=v, faces=f), 500, seed=4)['points'])
  cloud = mesh.sample_surface(dict(vertices=v[:600]), 7)                       # a cloud is its own sample, n is ignored
  assert torch.equal(cloud['points'], v[:600]) and torch.equal(cloud['face'].cpu(), torch.arange(600, dtype=torch.int32))


def test_sampling_is_stratified_in_the_area():
  verts, faces = small_mesh()
  n = 1001
  s = mesh.sample_surface(dict(vertices=dev(verts), faces=dev(faces)), n, seed=7)
  count = np.bincount(s['face'].cpu().numpy(), minlength=4)
  print('counts', count)
  assert count[1] == 0 and count[3] == 0 and count.sum() == n
  assert abs(count[0] - n / 4) <= 2 and abs(count[2] - 3 * n / 4) <= 2
  b = G.barycentrics(n, 7)
  assert (b >= 0).all() and (b <= 1).all() and (b.sum(1) == 1).all()
  z = s['points'].cpu().numpy()[:, 2]
  assert ((z == 0) == (s['face'].cpu().numpy() == 0)).all()


def test_sampling_is_uniform_on_a_face():
  verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
  faces = np.array([[0, 1, 2]], np.int32)
  n = 20000
  p = mesh.sample_surface(dict(vertices=dev(verts), faces=dev(faces)), n, seed=1)['points'].cpu().numpy().astype(np.float64)
  b = np.stack([1 - p[:, 0] - p[:, 1], p[:, 0], p[:, 1]], -1)                 # this face's barycentrics are its coordinates
  assert (b >= -1e-7).all() and (b <= 1 + 1e-7).all() and (p[:, 2] == 0).all()
  print('barycentric means', b.mean(0))
  assert np.abs(b.mean(0) - 1 / 3).max() <= 6 * np.sqrt(1 / (18 * n))


# ---- analytic

@functools.lru_cache(maxsize=None)
def sphere(bands, radius, half=False):
  m = R.latlong_sphere(bands, radius=radius)
  v, f = np.array(m['vertices']), np.array(m['faces'])
  if half:
    f = f[v[f].mean(1)[:, 2] > 0]
  e = np.concatenate([v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]], v[f[:, 2]] - v[f[:, 0]]]).astype(np.float64)
  h = np.linalg.norm(e, axis=-1).max()
  return v, f, radius - np.sqrt(radius ** 2 - h ** 2 / 3)                      # and the sagitta bound of its faces


def as_mesh(v, f):
  return dict(vertices=dev(v), faces=dev(f))


def test_distance_to_a_sphere():
  radius = 0.6
  v, f, sagitta = sphere(16, radius)
  rng = np.random.default_rng(31)
  d = rng.normal(size=(1000, 3))
  q = (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.05, 1.5, (1000, 1))).astype(np.float32)
  got = mesh.point_mesh_distance(dev(q), as_mesh(v, f))['distance'].cpu().numpy().astype(np.float64)
  exact = np.abs(np.linalg.norm(q.astype(np.float64), axis=-1) - radius)
  print(f'sphere: sagitta bound {sagitta:.4e}, largest deviation {np.abs(got - exact).max():.4e}')
  assert np.abs(got - exact).max() <= sagitta


# ---- metrics

N_SAMPLES = 6000


def test_metrics_of_a_mesh_against_itself():
  v, f, _ = sphere(12, 0.6)
  tol = 1e-5                                                                 # float32 distances of points ON a face of size 0.3: a few 1e-8
  r = mesh.geometry_metrics(as_mesh(v, f), as_mesh(v, f), n_samples=N_SAMPLES, thresholds=(tol, 1e-3, 0.1))
  print(r)
  assert all(isinstance(x, float) for x in r.values())
  for t in ('1e-05', '0.001', '0.1'):
    assert r[f'precision@{t}'] == r[f'recall@{t}'] == r[f'fscore@{t}'] == 1.
  assert 0 <= r['chamfer'] < tol and r['n_pred'] == r['n_gt'] == N_SAMPLES
  assert r['chamfer'] == 0.5 * (r['accuracy'] + r['completeness'])
  d = mesh.geometry_metrics(as_mesh(v, f), as_mesh(v, f), n_samples=500)     # default thresholds: from gt's box
  diag = float(np.linalg.norm(v.astype(np.float64).max(0) - v.astype(np.float64).min(0)))
  assert [k for k in d if k.startswith('fscore@')] == [f'fscore@{x * diag:g}' for x in mesh.GEOMETRY_THRESHOLDS]


def test_metrics_of_concentric_spheres():
  (v0, f0, s0), (v1, f1, s1) = sphere(24, 0.6), sphere(24, 0.65)
  timings = {}
  r = mesh.geometry_metrics(as_mesh(v0, f0), as_mesh(v1, f1), n_samples=N_SAMPLES, thresholds=(0.04, 0.06), timings=timings)
  print(r, 'sagitta', s0, s1, timings)
  assert abs(r['accuracy'] - 0.05) <= s0 + s1 and abs(r['completeness'] - 0.05) <= s0 + s1 and s0 + s1 < 0.009
  assert abs(r['accuracy_median'] - 0.05) <= s0 + s1 and abs(r['completeness_median'] - 0.05) <= s0 + s1
  assert r['fscore@0.04'] == 0. and r['precision@0.04'] == 0. and r['fscore@0.06'] == 1.
  assert set(timings) == {'sample', 'grid', 'query'} and all(t > 0 for t in timings.values())
  c = mesh.geometry_metrics(as_mesh(v0, f0), as_mesh(v1, f1), n_samples=N_SAMPLES, thresholds=(0.04,), max_dist=0.03)   # clamped
  assert all(c[k] == pytest.approx(0.03, abs=1e-9) for k in ('accuracy', 'completeness', 'chamfer', 'accuracy_median', 'completeness_median'))
  assert c['fscore@0.04'] == 1.
  cloud = mesh.geometry_metrics(as_mesh(v0, f0), dict(vertices=dev(v1)), n_samples=N_SAMPLES, thresholds=(0.04,))      # gt a point cloud
  assert cloud['n_gt'] == len(v1) and abs(cloud['completeness'] - 0.05) <= s0 + s1 and cloud['accuracy'] >= 0.05 - 1e-6


def test_metrics_of_half_a_sphere_are_asymmetric():
  v, f, s = sphere(24, 0.6)
  _, fh, _ = sphere(24, 0.6, half=True)
  keep = (v[f].mean(1)[:, 2] > 0).astype(int)
  runs = int((np.diff(keep) == 1).sum() + keep[0])                           # the kept faces are this many runs of consecutive ids
  tau = 0.01
  r = mesh.geometry_metrics(as_mesh(v, fh), as_mesh(v, f), n_samples=N_SAMPLES, thresholds=(tau,))
  share = G.face_areas(v, fh).sum() / G.face_areas(v, f).sum()
  print(r, 'area share', share)
  assert r['accuracy'] < 1e-5 and r['precision@0.01'] == 1.
  # recall: the gt samples ON the kept faces are within tau; those within tau of the rim besides: a band of area <= 2 pi R tau (1 + s / R)
  band = 2 * np.pi * 0.6 * tau * 1.05 / G.face_areas(v, f).sum()
  assert runs == 48 and 2 * runs / N_SAMPLES < 0.02         # stratified: a run of faces gets within 2 of its share of the samples
  assert share - 2 * runs / N_SAMPLES <= r['recall@0.01'] <= share + band + 2 * runs / N_SAMPLES
  assert r['completeness'] > 0.1 > r['accuracy'] and 0 < r['fscore@0.01'] < 1


def test_metrics_transform_and_bbox():
  v, f, _ = sphere(12, 0.6)
  shift = np.array([0.25, -0.5, 0.125], np.float32)                           # exact in float32, and so are the sums below to 1e-7
  moved = (v + shift).astype(np.float32)
  M = np.eye(4)
  M[:3, 3] = -shift
  off = mesh.geometry_metrics(as_mesh(moved, f), as_mesh(v, f), n_samples=2000, thresholds=(1e-4,))
  on = mesh.geometry_metrics(as_mesh(moved, f), as_mesh(v, f), n_samples=2000, thresholds=(1e-4,), transform=M)
  assert off['fscore@0.0001'] < 0.05 and off['chamfer'] > 0.1
  assert on['fscore@0.0001'] == 1. and on['chamfer'] < 1e-6
  # bbox: the upper half space only
  box = (-1, -1, 0, 1, 1, 1)
  _, fh, _ = sphere(12, 0.6, half=True)
  whole = mesh.geometry_metrics(as_mesh(v, fh), as_mesh(v, f), n_samples=2000, thresholds=(0.01,))
  cut = mesh.geometry_metrics(as_mesh(v, fh), as_mesh(v, f), n_samples=2000, thresholds=(0.01,), bbox=box)
  assert whole['recall@0.01'] < 0.6 and cut['recall@0.01'] == 1. and cut['n_gt'] < whole['n_gt'] == 2000 and cut['n_pred'] == 2000
  assert abs(cut['n_gt'] / 2000 - 0.5) < 0.05


# ---- eval_mesh.py

def run_eval(args):
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'eval_mesh.py')] + args, capture_output=True, text=True,
                     env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
  print(r.stdout[-3000:], r.stderr[-3000:])
  assert r.returncode == 0
  return r.stdout


def test_eval_mesh_script(tmp_path):
  """eval_mesh.py --geometry_only on two concentric spheres written with mesh.write_ply, with an error PLY; then without the new
  flags on the procedural dataset: exactly the files it wrote before."""
  (v0, f0, s0), (v1, f1, s1) = sphere(10, 0.6), sphere(24, 0.65)     # (10 bands: its vertices are not in the directions of gt's)
  pred, gt, err, out = (str(tmp_path / n) for n in ('pred.ply', 'gt.ply', 'error.ply', 'geo'))
  for path, v, f, r in ((pred, v0, f0, 0.6), (gt, v1, f1, 0.65)):
    mesh.write_ply(path, dict(vertices=v, normals=(v / r).astype(np.float32), faces=f))
  stdout = run_eval(['--mesh', pred, '--geometry_only', '--gt_mesh', gt, '--error_ply', err, '--out_dir', out, '--geometry_samples', '20000',
                     '--geometry_thresholds', '0.04,0.07'])
  assert os.listdir(out) == ['mesh_metric_geometry.txt'] and 'Geometry seconds: sample ' in stdout
  got = dict((l.split()[0], float(l.split()[1])) for l in open(os.path.join(out, 'mesh_metric_geometry.txt')).read().splitlines())
  want = mesh.geometry_metrics(as_mesh(v0, f0), as_mesh(v1, f1), n_samples=20000, thresholds=(0.04, 0.07))
  assert list(got) == list(want) and all(got[k] == pytest.approx(want[k], rel=1e-8) for k in want)
  assert abs(got['chamfer'] - 0.05) <= s0 + s1 and got['fscore@0.04'] == 0. and got['fscore@0.07'] == 1.
  assert all(f'{k} = ' in stdout for k in want)
  back = mesh.read_ply(err)
  assert np.array_equal(back['vertices'], v0) and np.array_equal(back['faces'], f0) and back['colors'].shape == (len(v0), 3)
  d = mesh.point_mesh_distance(dev(v0), as_mesh(v1, f1))['distance'].cpu().numpy()
  from matplotlib import colormaps
  lut = np.asarray(colormaps['turbo'](np.arange(256)))[:, :3]
  nearest = lut[np.clip(np.rint(d / 0.07 * 255).astype(int), 0, 255)] * 255
  assert np.abs(back['colors'].astype(np.float64) - nearest).max() <= 12      # one table step: the colour of the distance, 0 .. 0.07
  assert len(np.unique(back['colors'], axis=0)) > 1
  # without the new flags: what it wrote before
  ply = str(tmp_path / 'plain.ply')
  mesh.write_ply(ply, dict(vertices=(v0 / 0.6).astype(np.float32), normals=(v0 / 0.6).astype(np.float32), faces=f0))
  run_eval(['--mesh', ply, '--preset', 'blender_256', '--gin_bindings', "Config.dataset_loader = 'procedural'", '--gin_bindings', 'Config.factor = 2'])
  assert sorted(os.listdir(str(tmp_path / 'mesh_eval'))) == sorted(
      [f'mesh_color_{i:03d}.png' for i in range(6)] + ['mesh_metric_psnr.txt', 'mesh_metric_ssim.txt', 'mesh_render_times.txt'])
