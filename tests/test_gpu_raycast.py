"""Mesh ray casting on the GPU (-m gpu): the kernels of csrc/meshray.hip through ops.mesh_raycast / raycast_shade, mesh.cast_rays and
mesh.render_mesh(method='raycast') against the NumPy restatement (tests/raycast_ref.py, every ray against every face, no grid) bit for
bit; independence of the grid and of the order of the rays; watertightness from inside a closed sphere through a fisheye and a
panorama camera; the analytic sphere through every camera model; agreement with the rasteriser, whose buffers the shading kernel
reproduces bit for bit and whose default path must not have moved; argument checks and eval_mesh.py --method.
tests/test_raycast_cpu.py holds the restatement's own known answers."""

import functools
import os

import numpy as np
import pytest
import torch

from multinerf_amd import camera_utils, mesh, ops
from tests import raster_ref as R
from tests import raycast_ref as Q
from tests.test_gpu_raster import (BUFFERS, COLOUR_MODES, H, VIEWS, W, bits, colour_args, procedural, procedural_shading, projection,
                                   restated, run_eval, source, to_device, unit_sphere)

pytestmark = pytest.mark.gpu

F = np.float32
U24 = 2.0 ** -24
FISHEYE, PERSPECTIVE = camera_utils.ProjectionType.FISHEYE, camera_utils.ProjectionType.PERSPECTIVE
DISTORTION = dict(k1=0.08, k2=-0.03, p1=0.004, p2=-0.003)
PANO_EYE = (0.9, 0.5, 0.4)         # a panorama sees the sphere of radius 0.6 under 33 degrees from here: enough of its 32 x 64 rays hit


def dev(a, dtype=None):
  return torch.from_numpy(np.array(a, dtype=dtype, order='C')).cuda()      # (a copy: the shared sources are read-only)


def camera(view, h=H, w=W):
  eye, target, focal, near = VIEWS[view]
  return R.pixtocam(focal, w, h), R.look_at(eye, target), near


def view_rays(view, camtype=PERSPECTIVE, distortion=None, h=H, w=W):
  """(origins, directions) [h w,3] device tensors: the model's own rays of every pixel centre (camera_utils.pixels_to_rays)."""
  ptc, c2w, _ = camera(view, h, w)
  ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.int32).cuda(), torch.arange(w, dtype=torch.int32).cuda(), indexing='ij')
  o, d = camera_utils.pixels_to_rays(xs, ys, dev(ptc, F), dev(c2w, F), distortion_params=distortion, camtype=camtype)[:2]
  return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def free_rays(name, n=2000):
  """n rays (host, read-only) against mesh `name`, a tenth each: origins inside the box; origins 50 units away; axis-parallel
  directions; aimed exactly at vertices; at edge midpoints; at corners of the automatic grid's cells (origin + k cell); lying IN a
  grid plane; directions of length 1e-3; of length 1e3; and generic ones."""
  m = source(name)
  rng = np.random.default_rng(17)
  g = ops.mesh_grid_build(dev(m['vertices']), dev(m['faces']))
  org, cell, dims = np.array(g['origin'], F), F(g['cell']), np.array(g['dims'])
  k = n // 10
  o = rng.uniform(-0.6, 0.6, (n, 3))
  d = rng.normal(size=(n, 3))
  o[k:2 * k] = 50. * d[k:2 * k] / np.linalg.norm(d[k:2 * k], axis=-1, keepdims=True)
  d[k:2 * k] = rng.uniform(-0.5, 0.5, (k, 3)) - o[k:2 * k]
  axis = rng.integers(0, 3, k)
  d[2 * k:3 * k] = 0
  d[2 * k + np.arange(k), axis] = rng.choice([-1., 1., 0.37, -3.], k)
  o, d = o.astype(F), d.astype(F)
  ids = np.asarray(m['faces'])[rng.integers(0, len(m['faces']), 2 * k)]
  ids = np.where((ids >= 0) & (ids < len(m['vertices'])), ids, 0)
  vv = np.nan_to_num(m['vertices'][ids], nan=0.1, posinf=0.2, neginf=-0.2)
  d[3 * k:4 * k] = vv[:k, 0] - o[3 * k:4 * k]                                                   # a vertex (float32 difference)
  d[4 * k:5 * k] = (F(0.5) * (vv[k:, 0] + vv[k:, 1])) - o[4 * k:5 * k]                            # an edge midpoint
  corner = org + rng.integers(0, dims + 1, (k, 3)).astype(F) * cell
  d[5 * k:6 * k] = corner - o[5 * k:6 * k]
  plane = rng.integers(0, 3, k)                                                                 # in the plane x_a = origin_a + j cell
  rows = 6 * k + np.arange(k)
  o[rows, plane] = (org[plane] + rng.integers(0, dims[plane] + 1).astype(F) * cell)
  d[rows, plane] = 0
  scale = lambda x, s: (x / np.linalg.norm(x, axis=-1, keepdims=True) * s).astype(F)
  d[7 * k:8 * k], d[8 * k:9 * k] = scale(d[7 * k:8 * k], 1e-3), scale(d[8 * k:9 * k], 1e3)
  for a in (o, d):
    a.setflags(write=False)
  return o, d


@functools.lru_cache(maxsize=None)
def restated_cast(name, rays, cull='none', t_min=0., t_max=None):
  """The restatement's (t, face, bary) of a ray set ('outside' / 'inside': the view's pixel rays as the device builds them; 'free'),
  computed once and shared."""
  o, d = ray_set(name, rays)
  m = source(name)
  out = Q.cast(o, d, m['vertices'], m['faces'], t_min=t_min, t_max=np.inf if t_max is None else t_max, cull=cull)
  for a in out:
    a.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def ray_set(name, rays):
  if rays == 'free':
    return free_rays(name)
  o, d = view_rays(rays)
  return o.cpu().numpy(), d.cpu().numpy()


def cast(name, rays, **kw):
  m = source(name)
  o, d = ray_set(name, rays)
  return ops.mesh_raycast(dev(o), dev(d), dev(m['vertices']), dev(m['faces']), **kw)


def same(got, want):
  return all(np.array_equal(bits(g.cpu().numpy() if torch.is_tensor(g) else g), bits(w)) for g, w in zip(got, want))


# ---- bit equality

@pytest.mark.parametrize('rays', ['outside', 'inside', 'free'])
@pytest.mark.parametrize('name', ['soup', 'hand'])
def test_kernel_against_the_restatement(name, rays):
  """(t, face, bary) equal the restatement bit for bit, no exceptions: the soup has coincident, duplicated and reversed faces, the
  hand mesh NaN and infinite vertices, indices outside the vertices and faces without area."""
  want = restated_cast(name, rays)
  got = cast(name, rays, check_faces=False)
  assert [g.dtype for g in got] == [torch.float32, torch.int32, torch.float32] and tuple(got[2].shape) == (len(want[0]), 3)
  hit = want[1] >= 0
  print(f'{name} {rays}: {int(hit.sum())} of {len(hit)} rays hit')
  assert same(got, want)
  assert same(cast(name, rays, check_faces=False), want)                                         # two runs
  assert hit.sum() > (5 if name == 'hand' else 300) and ((~hit).sum() > 20 or (name, rays) == ('soup', 'inside'))
  assert (want[0][~hit] == np.inf).all() and (want[2][~hit] == 0).all()
  if name == 'hand':
    assert set(np.unique(want[1]).tolist()) <= {-1, 0, 1, 8}                                      # the six bad faces are never hit
  if name == 'soup' and rays != 'free':
    f = want[1]
    assert not ((f >= 50) & (f < 60)).any() and (rays == 'inside' or ((f >= 40) & (f < 50)).any())     # of identical faces the lower id


def test_degenerate_meshes_and_batches():
  m = source('soup')
  o, d = (dev(a) for a in free_rays('soup'))
  v, f = dev(m['vertices']), dev(m['faces'])
  # T = 1
  want = Q.cast(*free_rays('soup'), m['vertices'], m['faces'][7:8])
  assert same(ops.mesh_raycast(o, d, v, f[7:8].contiguous()), want) and (want[1] == 0).sum() > 3
  # no faces, no vertices, no rays
  empty = lambda r, n: (tuple(r[0].shape) == (n,) and tuple(r[2].shape) == (n, 3) and bool((r[0] == float('inf')).all()) and
                        bool((r[1] == -1).all()) and bool((r[2] == 0).all()))
  none = torch.zeros((0, 3), dtype=torch.int32).cuda()
  assert empty(ops.mesh_raycast(o, d, v, none), len(o)) and empty(ops.mesh_raycast(o, d, torch.zeros((0, 3)).cuda(), none), len(o))
  assert empty(ops.mesh_raycast(o[:0], d[:0], v, f), 0)
  r = mesh.cast_rays(dict(vertices=v, faces=none), o, d)
  assert bool((r['face'] == -1).all()) and bool((r['normals'] == 0).all())
  # every face invalid: an empty grid
  bad = torch.full((4, 3), -1, dtype=torch.int32).cuda()
  assert empty(ops.mesh_raycast(o, d, v, bad, check_faces=False), len(o))
  # rays that are not finite, and d = 0, among good ones
  o2, d2 = o[:64].clone(), d[:64].clone()
  o2[3, 1], d2[5, 0], d2[9, 2], d2[11] = float('nan'), float('inf'), float('nan'), 0.
  want = Q.cast(o2.cpu().numpy(), d2.cpu().numpy(), m['vertices'], m['faces'])
  assert same(ops.mesh_raycast(o2, d2, v, f), want) and (want[1][[3, 5, 9, 11]] == -1).all() and (want[1] >= 0).sum() > 10


# ---- the result does not depend on the grid or the order

@pytest.mark.parametrize('name', ['soup', 'latlong'])
def test_grid_and_order_independence(name):
  m = source(name)
  v, f = dev(m['vertices']), dev(m['faces'])
  auto = ops.mesh_grid_build(v, f)
  for rays in ('outside', 'free'):
    o, d = (dev(a) for a in ray_set(name, rays))
    base = ops.mesh_raycast(o, d, v, f, grid=auto)
    assert same(base, restated_cast(name, rays)) and int((base[1] >= 0).sum()) > 300
    for factor in (0.37, 4., 1e3):                                                               # finer, coarser, one single cell
      grid = ops.mesh_grid_build(v, f, cell=factor * auto['cell'])
      assert (grid['dims'] == [1, 1, 1] if factor == 1e3 else grid['dims'] != auto['dims'] or auto['dims'] == [1, 1, 1]), (factor, grid['dims'])
      assert all(torch.equal(a, b) for a, b in zip(ops.mesh_raycast(o, d, v, f, grid=grid), base)), (rays, factor)
    assert all(torch.equal(a, b) for a, b in zip(ops.mesh_raycast(o, d, v, f, cell=0.37 * auto['cell']), base))
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(o))).cuda()
    shuffled = ops.mesh_raycast(o[perm].contiguous(), d[perm].contiguous(), v, f, grid=auto)
    assert all(torch.equal(a, b[perm]) for a, b in zip(shuffled, base))
    orders = [torch.arange(len(o)).cuda(), perm.contiguous()] + ([ops.pixel_tile_order(H, W, o.device)] if rays == 'outside' else [])
    for order in orders:                                                                         # row-major, random, 8 x 8 tiles
      assert sorted(order.tolist()) == list(range(len(o)))
      assert all(torch.equal(a, b) for a, b in zip(ops.mesh_raycast(o, d, v, f, grid=auto, order=order), base))


# ---- watertightness

def pano_rays(eye, h, w):
  c2w = dev(R.look_at(eye, (1., 0.3, 0.2)), F)
  o, d = ops.spherical_rays(c2w, h, w)[:2]
  return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def test_watertight_from_inside_the_closed_sphere():
  """From the eye of view `inside`, within the closed marching-tetrahedra sphere (10,364 faces): every one of the 47 x 61 rays of a
  fisheye camera and of the 32 x 64 rays of a panorama hits, and so does every ray aimed at one of 500 vertices and 500 edge
  midpoints (float32 differences: the ray passes within rounding of the vertex or edge, which all the faces around it share)."""
  m = source('sphere')
  assert len(m['faces']) == 10364
  v, f = dev(m['vertices']), dev(m['faces'])
  grid = ops.mesh_grid_build(v, f)
  eye = VIEWS['inside'][0]
  for label, (o, d) in (('fisheye', view_rays('inside', camtype=FISHEYE)), ('pano', pano_rays(eye, 32, 64))):
    t, face, bary = ops.mesh_raycast(o, d, v, f, grid=grid)
    spread = d / d.norm(dim=-1, keepdim=True)
    print(f'{label}: {len(o)} rays, {int((face >= 0).sum())} hit, direction spread {spread.min(0).values.tolist()} .. {spread.max(0).values.tolist()}')
    assert bool((face >= 0).all()) and bool(torch.isfinite(t).all()) and len(torch.unique(face)) > 100
    assert bool(((bary >= 0).all(-1) & ((bary.sum(-1) - 1).abs() < 1e-5)).all())
  assert float((pano_rays(eye, 32, 64)[1].max(0).values - pano_rays(eye, 32, 64)[1].min(0).values).min()) > 1.5       # all around
  rng = np.random.default_rng(23)
  o = np.broadcast_to(np.asarray(eye, F), (1000, 3))
  ids = m['faces'][rng.choice(len(m['faces']), 1000, replace=False)]
  target = np.concatenate([m['vertices'][ids[:500, 0]], F(0.5) * (m['vertices'][ids[500:, 1]] + m['vertices'][ids[500:, 2]])])
  t, face, bary = ops.mesh_raycast(dev(o), dev((target - o).astype(F)), v, f, grid=grid)
  assert bool((face >= 0).all()) and bool(((t - 1).abs() < 1e-4).all())                          # the target is the hit: t = 1
  assert same((t, face, bary), Q.cast(o, (target - o).astype(F), m['vertices'], m['faces']))


# ---- the analytic sphere, every camera model

def plane_radius(m):
  """r_in: the smallest distance from the origin to the plane of a face, float64 (no point of the mesh is nearer)."""
  v = m['vertices'].astype(np.float64)[m['faces']]
  n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
  return float(np.abs((n * v[:, 0]).sum(-1) / np.linalg.norm(n, axis=-1)).min())


@pytest.mark.parametrize('model', ['perspective', 'distorted', 'fisheye', 'pano'])
def test_analytic_sphere_through_every_camera_model(model):
  """latlong_sphere(12) of radius 0.6 (vertices on the sphere to float32 rounding) from the eye of view `outside` (the panorama: from PANO_EYE).  With r_in the
  smallest origin-to-face-plane distance (float64), every hit point satisfies r_in - e <= |o + t d| <= 0.6 + e, every ray whose exact
  closest approach to the centre is below r_in - e hits and every ray above 0.6 + e misses.  e = 12 sqrt(3) u (max_a |o_a| + 0.6) +
  0.6 * 2^-23, u = 2^-24: the distance of the computed hit point from its face that csrc/meshray.hip derives (12 u M in the maximum
  norm, M <= max_a |o_a| + 0.6), and the rounding of the vertices onto the sphere.  render_mesh's depth is that t."""
  m = source('latlong')
  dm = to_device(m)
  r_in = plane_radius(m)
  assert 0.58 < r_in < 0.6
  ptc, c2w, near = camera('outside')
  h, w = (32, 64) if model == 'pano' else (H, W)
  if model == 'pano':
    c2w = R.look_at(PANO_EYE, (0., 0., 0.))
  kw = dict(perspective={}, distorted=dict(distortion_params=DISTORTION), fisheye=dict(camtype=FISHEYE), pano=dict(camtype='pano'))[model]
  r = mesh.render_mesh(dm, ptc, c2w, h, w, near=near, method='raycast', **kw)
  assert r['proj'] is None and tuple(r['depth'].shape) == (h, w) and tuple(r['rgb'].shape) == (h, w, 3)
  if model == 'pano':
    o, d = (x.reshape(-1, 3).contiguous() for x in ops.spherical_rays(dev(c2w, F), h, w)[:2])
  else:
    o, d = view_rays('outside', camtype=kw.get('camtype', PERSPECTIVE), distortion=kw.get('distortion_params'))
  t, face, bary = ops.mesh_raycast(o, d, dm['vertices'], dm['faces'], t_min=near)
  hit = (face >= 0).reshape(h, w)
  assert torch.equal(r['face'], face.reshape(h, w)) and torch.equal(r['bary'], bary.reshape(h, w, 3)) and torch.equal(r['acc'], hit.float())
  assert torch.equal(r['depth'], torch.where(hit, t.reshape(h, w), torch.zeros(()).cuda()))       # depth equals t (0 on a miss)
  o64, d64, t64 = o.cpu().numpy().astype(np.float64), d.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
  hit = hit.reshape(-1).cpu().numpy()
  e = 12 * np.sqrt(3) * U24 * (np.abs(o64).max() + 0.6) + 0.6 * 2.0 ** -23
  radius = np.linalg.norm(o64[hit] + t64[hit, None] * d64[hit], axis=-1)
  s = -(o64 * d64).sum(-1) / (d64 * d64).sum(-1)                                                  # the parameter of the closest approach
  closest = np.linalg.norm(o64 + np.maximum(s, 0)[:, None] * d64, axis=-1)
  must, must_not = closest < r_in - e, closest > 0.6 + e
  print(f'{model}: {int(hit.sum())} of {len(hit)} rays hit, {int(must.sum())} must, {int(must_not.sum())} must not, |o + t d| in '
        f'[{radius.min():.7f}, {radius.max():.7f}] of [{r_in - e:.7f}, {0.6 + e:.7f}], e = {e:.2e}')
  assert must.sum() > 30 and must_not.sum() > 200 and hit[must].all() and not hit[must_not].any()
  assert radius.min() >= r_in - e and radius.max() <= 0.6 + e


# ---- agreement with the rasteriser

def test_raycast_against_the_rasteriser():
  """render_mesh(method='raycast') against method='raster' on view `outside`, pinhole: the faces differ at no more than 1 % of the pixels
  (tests/test_raycast_cpu.py verifies the cap on the two restatements); the shading kernel, given the RASTERISER's face and bary, returns
  the rasteriser's rgb and normals bit for bit, with vertex colours, with a texture and with neither; and method='raster' and the
  default return what the restatement of the rasteriser says, bit for bit, as they did before there was a method."""
  m = source('latlong')
  dm = to_device(m)
  ptc, c2w, near = camera('outside')
  ray = mesh.render_mesh(dm, ptc, c2w, H, W, near=near, method='raycast')
  for mode in COLOUR_MODES:
    _, dev_kw = colour_args(m, mode)
    want = restated('latlong', 'outside', mode)
    render_kw = {}
    if 'colors' in dev_kw:
      render_kw = dict(colors=dev_kw['colors'])
    if 'texture' in dev_kw:
      render_kw = dict(texture=dev_kw)
    for kw in ({}, dict(method='raster'), dict(method='auto')):
      ras = mesh.render_mesh(dm, ptc, c2w, H, W, near=near, **render_kw, **kw)
      assert np.array_equal(ras['proj'], projection('outside')[0])
      assert all(np.array_equal(bits(ras[k].cpu().numpy()), bits(want[k])) for k in BUFFERS), (mode, kw)
    out = ops.raycast_shade(dm, ras['face'], ras['bary'], **dev_kw)
    assert torch.equal(out['rgb'], ras['rgb']) and torch.equal(out['normals'], ras['normals']), mode
    flat = ops.raycast_shade(dm, ras['face'].reshape(-1), ras['bary'].reshape(-1, 3), bg=(0.25, 0.5, 0.75), **dev_kw)
    miss = ras['face'].reshape(-1) < 0
    assert torch.equal(flat['rgb'][~miss], ras['rgb'].reshape(-1, 3)[~miss]) and bool((flat['rgb'][miss] == torch.tensor([0.25, 0.5, 0.75]).cuda()).all())
  ras = mesh.render_mesh(dm, ptc, c2w, H, W, near=near)
  differ = (ray['face'] != ras['face'])
  print(f'{int(differ.sum())} of {H * W} pixels differ; {int((ray["face"] >= 0).sum())} hit')
  assert float(differ.float().mean()) <= 0.01 and int((ray['face'] >= 0).sum()) > 200
  agree = ~differ & (ras['face'] >= 0)
  assert float(((ray['depth'] - ras['depth']).abs() / ras['depth'].clamp(min=1e-6))[agree].max()) <= 1e-3
  assert float((ray['rgb'] - ras['rgb']).abs()[agree].max()) <= 5e-3 and torch.equal(ray['acc'][~differ], ras['acc'][~differ])


# ---- the other cases

def test_cull_back_against_the_restatement():
  for name, rays in (('soup', 'outside'), ('soup', 'free'), ('latlong', 'outside')):
    want = restated_cast(name, rays, cull='back')
    assert same(cast(name, rays, cull='back', check_faces=False), want)
    assert (want[1] >= 0).sum() > 300 and not same(want, restated_cast(name, rays)) or name == 'latlong'
  # the closed sphere, counter-clockwise seen from outside: from outside cull changes nothing, from inside nothing is left
  assert same(restated_cast('latlong', 'outside', cull='back'), restated_cast('latlong', 'outside'))
  inside = cast('latlong', 'inside', cull='back')
  assert bool((inside[1] == -1).all()) and bool((cast('latlong', 'inside')[1] >= 0).all())
  # t_min and t_max against the restatement
  want = restated_cast('soup', 'free', t_min=0.25, t_max=1.5)
  assert same(cast('soup', 'free', t_min=0.25, t_max=1.5), want) and (want[1] >= 0).sum() > 100 and not same(want, restated_cast('soup', 'free'))


def test_supersample_shapes_and_box_average():
  m = source('latlong')
  dm = to_device(m)
  ptc, c2w, near = camera('outside')
  for kw, (h, w) in ((dict(), (H, W)), (dict(camtype='pano'), (16, 32))):
    k = 2
    if kw:
      c2w = R.look_at(PANO_EYE, (0., 0., 0.))
    s = mesh.render_mesh(dm, ptc, c2w, h, w, near=near, method='raycast', supersample=k, **kw)
    fine = mesh.render_mesh(dm, ptc @ np.diag([1. / k, 1. / k, 1.]), c2w, k * h, k * w, near=near, method='raycast', **kw)
    assert tuple(s['face'].shape) == (k * h, k * w) and tuple(s['rgb'].shape) == (h, w, 3) and tuple(s['acc'].shape) == (h, w)
    assert all(torch.equal(s[n], fine[n]) for n in ('face', 'depth', 'bary', 'normals'))
    acc = fine['acc'].cpu().numpy().astype(np.float64).reshape(h, k, w, k).mean((1, 3))
    rgb = fine['rgb'].cpu().numpy().astype(np.float64).reshape(h, k, w, k, 3).mean((1, 3))
    assert np.abs(s['acc'].cpu().numpy() - acc).max() <= 1e-6 and np.abs(s['rgb'].cpu().numpy() - rgb).max() <= 1e-6
    assert ((acc > 0) & (acc < 1)).sum() > (3 if kw else 10)                                     # the silhouette is anti-aliased


def test_sh_texture_through_the_raycast_path():
  m = source('latlong')
  dm = to_device(m)
  ptc, c2w, near = camera('outside')
  rng = np.random.default_rng(31)
  tex = dict(texture=dev(m['texture']), uv=dev(m['uv']), sh=dev(rng.normal(0.3, 0.3, (13, 17, 9, 3)).astype(F)))
  r = mesh.render_mesh(dm, ptc, c2w, H, W, near=near, method='raycast', texture=tex, camtype=FISHEYE)
  plain = mesh.render_mesh(dm, ptc, c2w, H, W, near=near, method='raycast', texture=tex, camtype=FISHEYE, view_dependent=False)
  want = ops.shtex_shade(dm, r['face'], r['bary'], tex['uv'], tex['sh'], VIEWS['outside'][0], plain['rgb'].clone())
  assert torch.equal(r['rgb'], want) and not torch.equal(r['rgb'], plain['rgb']) and torch.equal(r['face'], plain['face'])
  assert torch.equal(plain['rgb'], ops.raycast_shade(dm, r['face'], r['bary'], texture=tex['texture'], uv=tex['uv'])['rgb'])


def test_auto_picks_the_method_by_the_camera():
  m = source('latlong')
  dm = to_device(m)
  ptc, c2w, near = camera('outside')
  assert mesh.render_mesh(dm, ptc, c2w, H, W, near=near, method='auto')['proj'] is not None
  for kw in (dict(camtype=FISHEYE), dict(camtype='pano'), dict(distortion_params=DISTORTION), dict(pixtocam_ndc=ptc)):
    assert not mesh.camera_is_pinhole(**kw)
    auto, ray = (mesh.render_mesh(dm, ptc, c2w, H, W, near=near, method=method, **kw) for method in ('auto', 'raycast'))
    assert auto['proj'] is None and all(torch.equal(auto[k], ray[k]) for k in BUFFERS)
    with pytest.raises(ValueError):
      mesh.render_mesh(dm, ptc, c2w, H, W, near=near, **kw)                                       # the rasteriser still refuses them
  assert mesh.camera_is_pinhole() and mesh.camera_is_pinhole(camtype=PERSPECTIVE)
  # with pixtocam_ndc the rays are the world-space ones
  a, b = (mesh.render_mesh(dm, ptc, c2w, H, W, near=near, method='raycast', **kw) for kw in ({}, dict(pixtocam_ndc=ptc)))
  assert all(torch.equal(a[k], b[k]) for k in BUFFERS)


def test_cast_rays_returns_points_and_face_normals():
  m = {k: np.array(v) for k, v in source('latlong').items()}                                      # (copies: the shared source is read-only)
  o, d = free_rays('latlong')
  r = mesh.cast_rays(m, o.reshape(40, 50, 3).copy(), d.reshape(40, 50, 3).copy())
  assert [tuple(r[k].shape) for k in ('t', 'face', 'bary', 'points', 'normals')] == [(40, 50), (40, 50), (40, 50, 3), (40, 50, 3), (40, 50, 3)]
  want = restated_cast('latlong', 'free')
  assert same((r['t'].reshape(-1), r['face'].reshape(-1), r['bary'].reshape(-1, 3)), want)
  hit = want[1] >= 0
  p = r['points'].reshape(-1, 3).cpu().numpy()[hit]
  assert hit.sum() > 300 and np.abs(np.linalg.norm(p, axis=-1) - 0.6).max() < 0.011               # on the sphere (sagitta of 12 bands)
  n = r['normals'].reshape(-1, 3).cpu().numpy()
  assert (n[~hit] == 0).all() and np.abs(np.linalg.norm(n[hit], axis=-1) - 1).max() < 1e-6 and ((n[hit] * p).sum(-1) > 0).all()
  # t_max as an occlusion test: from outside, a point on the far side of the sphere is blocked, one on the near side is not
  eye = np.asarray(VIEWS['outside'][0], F)
  far, near_pt = -0.6 * eye / np.linalg.norm(eye), 0.7 * eye / np.linalg.norm(eye)
  blocked = mesh.cast_rays(m, np.stack([eye, eye]), np.stack([far - eye, near_pt - eye]).astype(F), t_max=0.999)['face']
  assert int(blocked[0]) >= 0 and int(blocked[1]) == -1


def test_argument_checks():
  m = source('soup')
  v, f = dev(m['vertices']), dev(m['faces'])
  o, d = (dev(a) for a in free_rays('soup'))
  dm = to_device(source('latlong'))
  other = ops.mesh_grid_build(dm['vertices'], dm['faces'])                                         # 528 faces: not the soup's 300
  grid = ops.mesh_grid_build(v, f)
  ok = ops.mesh_raycast(o, d, v, f, grid=grid)
  face, bary = torch.zeros((5,), dtype=torch.int32).cuda(), torch.zeros((5, 3)).cuda()
  cases = [
      lambda: ops.mesh_raycast(o.double(), d, v, f),
      lambda: ops.mesh_raycast(o, d.half(), v, f),
      lambda: ops.mesh_raycast(o, d[:-1], v, f),
      lambda: ops.mesh_raycast(o.reshape(-1), d.reshape(-1), v, f),
      lambda: ops.mesh_raycast(o, d, v.double(), f),
      lambda: ops.mesh_raycast(o, d, v, f.long()),
      lambda: ops.mesh_raycast(o, d, v, f.reshape(-1, 2)),
      lambda: ops.mesh_raycast(o, d, v[:100], f),                                                 # indices outside the vertices
      lambda: ops.mesh_raycast(o, d, v, f, t_min=-0.1),
      lambda: ops.mesh_raycast(o, d, v, f, t_min=float('nan')),
      lambda: ops.mesh_raycast(o, d, v, f, t_min=float('inf')),
      lambda: ops.mesh_raycast(o, d, v, f, t_min=1., t_max=1.),
      lambda: ops.mesh_raycast(o, d, v, f, t_min=1., t_max=0.5),
      lambda: ops.mesh_raycast(o, d, v, f, t_max=float('nan')),
      lambda: ops.mesh_raycast(o, d, v, f, cull='front'),
      lambda: ops.mesh_raycast(o, d, v, f, grid=other),                                           # a grid of another mesh
      lambda: ops.mesh_raycast(o, d, v, f, grid=dict(grid, dims=[1, 1, 1])),
      lambda: ops.mesh_raycast(o, d, v, f, grid=grid, cell=0.1),
      lambda: ops.mesh_raycast(o, d, v, f, cell=0.),
      lambda: ops.mesh_raycast(o, d, v, f, order=torch.arange(len(o), dtype=torch.int32).cuda()),
      lambda: ops.mesh_raycast(o, d, v, f, order=torch.arange(len(o) - 1).cuda()),
      lambda: ops.raycast_shade(dm, face.long(), bary),
      lambda: ops.raycast_shade(dm, face, bary.double()),
      lambda: ops.raycast_shade(dm, face, bary[:4]),
      lambda: ops.raycast_shade(dm, face, bary, colors=torch.zeros((5, 3), dtype=torch.uint8).cuda()),
      lambda: ops.raycast_shade(dm, face, bary, texture=torch.zeros((4, 4, 3)).cuda()),
      lambda: ops.raycast_shade(dm, face, bary, uv=torch.zeros((528, 3, 2)).cuda()),
      lambda: ops.raycast_shade(dm, face, bary, bg=(1., 1.)),
      lambda: ops.raycast_shade(dict(dm, normals=dm['normals'][:-1]), face, bary),
      lambda: mesh.cast_rays(source('latlong'), np.zeros((4, 3), F), np.zeros((5, 3), F)),
      lambda: mesh.render_mesh(dm, None, None, H, W, proj=projection('outside')[0], method='raycast'),
      lambda: mesh.render_mesh(dm, *camera('outside')[:2], H, W, method='rays'),
      lambda: mesh.render_mesh(dm, *camera('outside')[:2], H, W, method='raycast', near=0.),
      lambda: mesh.render_mesh(dm, *camera('outside')[:2], H, W, method='raycast', cull='front'),
      lambda: mesh.render_mesh(dm, *camera('outside')[:2], H, W, method='raycast', supersample=0),
  ]
  if os.environ.get('MNR_TESTS_ON_SIMULATOR') != '1':       # (on the simulator every tensor is a host tensor)
    cases.append(lambda: ops.mesh_raycast(o.cpu(), d.cpu(), v, f))
  for n, case in enumerate(cases):
    with pytest.raises(ValueError):
      case()
      print('case', n, 'did not raise')
  assert all(torch.equal(a, b) for a, b in zip(ops.mesh_raycast(o, d, v, f, grid=grid), ok))      # and nothing was disturbed


# ---- eval_mesh.py

def test_eval_mesh_script_methods(tmp_path):
  """eval_mesh.py on the procedural preset at factor 2 (six 48 x 48 pinhole test views) with a sphere coloured per vertex: --method
  raycast writes the same files as --method raster and its 8-bit images differ from the rasteriser's at no more than 1 % of the
  pixels; the default run (auto) says it rasterises and its files are byte for byte those of --method raster.  The procedural loader
  takes a camera model through gin only as Config.render_camtype, which needs Config.render_path = True, and a render path has no
  images: a fisheye and a 'pano' run are therefore rendered end to end (the default method must pick the ray caster) but cannot be
  SCORED; the camera-model coverage of the values rests on the render_mesh cases above."""
  from PIL import Image
  config, dataset = procedural('test')
  m = unit_sphere()
  m['colors'] = np.floor(np.clip(procedural_shading(m['vertices'].astype(np.float64)), 0, 1) * 255 + 0.5).astype(np.uint8)
  binds = ['--preset', 'blender_256', '--gin_bindings', "Config.dataset_loader = 'procedural'", '--gin_bindings', 'Config.factor = 2']
  ply = str(tmp_path / 'sphere.ply')
  mesh.write_ply(ply, m)
  outs = {}
  for method in ('raster', 'raycast', 'auto'):
    out_dir = str(tmp_path / method)
    stdout = run_eval(['--mesh', ply, '--out_dir', out_dir] + ([] if method == 'auto' else ['--method', method]) + binds)
    assert f'rendering method: {"raster" if method == "auto" else method}' in stdout
    outs[method] = out_dir
  names = sorted(os.listdir(outs['raster']))
  assert names == sorted(os.listdir(outs['raycast'])) == sorted(os.listdir(outs['auto'])) and len(names) == 6 + 3
  for name in names:
    a, b = (open(os.path.join(outs[k], name), 'rb').read() for k in ('raster', 'auto'))
    assert a == b or name == 'mesh_render_times.txt', name
  differ = total = 0
  for name in (n for n in names if n.endswith('.png')):
    a, b = (np.asarray(Image.open(os.path.join(outs[k], name))) for k in ('raster', 'raycast'))
    assert a.shape == b.shape == (48, 48, 3)
    differ, total = differ + int((a != b).any(-1).sum()), total + a.shape[0] * a.shape[1]
  print(f'{differ} of {total} pixels differ between the rasteriser and the ray caster')
  assert differ <= 0.01 * total
  pr, pc = ([float(v) for v in open(os.path.join(outs[k], 'mesh_metric_psnr.txt')).read().split()] for k in ('raster', 'raycast'))
  assert len(pr) == len(pc) == 6 and max(abs(a - b) for a, b in zip(pr, pc)) < 0.5
  path = ['--gin_bindings', 'Config.render_path = True', '--gin_bindings', 'Config.render_path_frames = 3']
  for camtype in ('fisheye', 'pano'):
    out_dir = str(tmp_path / camtype)
    stdout = run_eval(['--mesh', ply, '--out_dir', out_dir, '--gin_bindings', f"Config.render_camtype = '{camtype}'"] + path + binds)
    assert 'rendering method: raycast (chosen by the cameras)' in stdout
    assert sorted(os.listdir(out_dir)) == [f'mesh_color_{i:03d}.png' for i in range(3)] + ['mesh_render_times.txt']
    png = np.asarray(Image.open(os.path.join(out_dir, 'mesh_color_001.png')))
    assert png.shape == (48, 48, 3) and (png != 255).any(-1).sum() > 20 and (png == 255).all(-1).sum() > 50      # the sphere, on white
