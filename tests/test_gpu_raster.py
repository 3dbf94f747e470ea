"""Mesh rasteriser on the GPU (-m gpu): the kernels of csrc/raster.hip through ops.raster_visibility / raster_shade and
mesh.render_mesh against the NumPy restatement (tests/raster_ref.py, every face against every pixel) bit for bit, watertightness on
the kernels' own cover counts, the projection and `front` conventions, the analytic sphere of the `procedural` dataset, the atlas's
seam claim by rendering, a TSDF round trip, argument checks, degenerate inputs and eval_mesh.py.  tests/test_raster_cpu.py holds the
restatement's own known answers."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import mesh_clean_ref as C
from tests import raster_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 47, 61                      # no multiples of the workgroup (256 pixels), of a wave or of each other
HUGE = 1 << 40
BUFFERS = ('face', 'depth', 'acc', 'bary', 'normals', 'rgb')


def to_device(m):
  return {k: torch.from_numpy(np.array(m[k])).cuda() for k in ('vertices', 'normals', 'faces')}


def bits(a):
  a = np.ascontiguousarray(a)
  return a.view(np.uint32) if a.dtype == np.float32 else a


def host(out):
  return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def soup(T=300, seed=5):
  """Random triangles in [-0.6, 0.6]^3 that intersect each other; the last 40 repeat the first 40 with the opposite winding
  (coincident faces whose depths agree to rounding only: det and S are summed in another order, so either may win a pixel, and the
  kernels must pick the one the restatement picks) and faces 50 .. 59 repeat 40 .. 49 as they are (equal depth bits: the lower id
  wins)."""
  rng = np.random.default_rng(seed)
  verts = rng.uniform(-0.6, 0.6, (3 * T, 3)).astype(np.float32)
  faces = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
  faces[50:60] = faces[40:50]
  faces[T - 40:] = faces[:40, ::-1]
  return dict(vertices=verts, normals=rng.normal(size=(3 * T, 3)).astype(np.float32), faces=faces)


def hand():
  """12 vertices, 9 faces: 0, 1 ordinary (1 with zero vertex normals: the face normal takes over), 2 zero area (two equal corners),
  3 three collinear corners, 4 with a NaN vertex, 5 with an infinite one, 6 and 7 with an index outside the vertices (-1 and V),
  8 ordinary and large."""
  v = np.array([[-.5, -.4, 0.], [.5, -.4, .1], [0., .5, -.1], [-.3, .2, .3], [.4, .3, .3], [.1, -.5, .35], [0., 0., .2], [.2, .2, .2],
                [np.nan, 0., 0.], [np.inf, .1, .1], [-.6, .6, -.3], [.6, .6, -.3]], np.float32)
  n = np.random.default_rng(9).normal(size=v.shape).astype(np.float32)
  n[3:6] = 0
  f = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 1], [6, 7, 6], [0, 8, 2], [9, 1, 2], [-1, 1, 2], [0, 12, 2], [10, 0, 11]], np.int32)
  f[3] = (0, 6, 7)
  v[6], v[7] = v[0] * 0.5, v[0] * 0.25                       # 0, 6, 7 on one line through the origin
  return dict(vertices=v, normals=n, faces=f)


@functools.lru_cache(maxsize=None)
def source(name):
  if name == 'sphere':
    m = dict(C.source_mesh('sphere')[0])                    # marching tetrahedra, radius 0.6, 10364 faces
  elif name == 'latlong':
    m = R.latlong_sphere(12, radius=0.6)
  else:
    m = dict(soup=soup, hand=hand)[name]()
  m = {k: np.array(m[k]) for k in ('vertices', 'normals', 'faces')}
  rng = np.random.default_rng(len(m['faces']))
  m['colors'] = rng.integers(0, 256, m['vertices'].shape).astype(np.uint8)
  m['texture'] = rng.integers(0, 256, (13, 17, 3)).astype(np.uint8)
  m['uv'] = rng.uniform(-0.1, 1.1, (len(m['faces']), 3, 2)).astype(np.float32)      # beyond [0, 1]: the clamps
  for a in m.values():
    a.setflags(write=False)
  return m


# eye, target, focal, near
VIEWS = {
    'outside': ((2.0, 1.2, 0.8), (0.02, -0.03, 0.01), 90., 1e-3),
    'inside': ((0.1, -0.05, 0.15), (1., 0.3, 0.2), 20., 1e-3),
    'near_cut': ((2.0, 1.2, 0.8), (0.02, -0.03, 0.01), 90., 2.45),             # |eye| = 2.47: the near plane cuts through the mesh
}


def projection(view, h=H, w=W):
  eye, target, focal, near = VIEWS[view]
  return mesh.world_to_pixel(R.pixtocam(focal, w, h), R.look_at(eye, target)), near


COLOUR_MODES = ('normals', 'colors_u8', 'colors_f32', 'texture_u8', 'texture_f32')


def colour_args(m, mode):
  """(kwargs of the restatement, kwargs of ops.raster_shade) of a colour source."""
  if mode == 'normals':
    return {}, {}
  kind, dtype = mode.split('_')
  if kind == 'colors':
    c = m['colors'] if dtype == 'u8' else (m['colors'].astype(np.float32) / np.float32(255)) ** 2
    return dict(colors=c), dict(colors=torch.from_numpy(np.array(c)).cuda())
  t = m['texture'] if dtype == 'u8' else (m['texture'].astype(np.float32) / np.float32(255)) ** 2
  return dict(texture=t, uv=m['uv']), dict(texture=torch.from_numpy(np.array(t)).cuda(), uv=torch.from_numpy(np.array(m['uv'])).cuda())


@functools.lru_cache(maxsize=None)
def restated(name, view, mode='normals'):
  """The restatement's buffers, computed once and shared (the visibility buffer once per mesh and view)."""
  m = source(name)
  P, near = projection(view)
  if mode == 'normals':
    out = R.render(m, P, H, W, near)
  else:
    out = R.shade(m['vertices'], m['normals'], m['faces'], P, restated(name, view)['vis'], near, **colour_args(m, mode)[0])
  for a in out.values():
    a.setflags(write=False)
  return out


# ---- against the restatement

@pytest.mark.parametrize('view', list(VIEWS))
@pytest.mark.parametrize('name', ['latlong', 'soup', 'hand', 'sphere'])
def test_kernels_against_the_restatement(name, view):
  m = source(name)
  dm = to_device(m)
  P, near = projection(view)
  want = restated(name, view)
  vis = {t: ops.raster_visibility(dm, P, H, W, near, threshold=t, check_faces=False) for t in (0, None, HUGE)}
  assert vis[None].dtype == torch.int64 and tuple(vis[None].shape) == (H, W)
  got = vis[None].cpu().numpy().view(np.uint64)
  covered = int((got != R.EMPTY).sum())
  print(f'{name} {view}: {len(m["faces"])} faces, {covered} of {H * W} pixels covered')
  assert np.array_equal(got, want['vis'])
  assert torch.equal(vis[0], vis[None]) and torch.equal(vis[HUGE], vis[None])                       # all large = default = all small
  assert torch.equal(ops.raster_visibility(dm, P, H, W, near, check_faces=False), vis[None])        # two runs
  if name != 'hand':
    assert covered > 200
  for mode in COLOUR_MODES:
    ref_kw, dev_kw = colour_args(m, mode)
    ref = restated(name, view, mode)
    out = ops.raster_shade(dm, P, vis[None], near, bg=(0.25, 0.5, 0.75) if mode == 'colors_u8' else (1., 1., 1.), **dev_kw)
    assert [out[k].dtype for k in BUFFERS] == [torch.int32] + [torch.float32] * 5
    assert [tuple(out[k].shape) for k in BUFFERS] == [(H, W), (H, W), (H, W), (H, W, 3), (H, W, 3), (H, W, 3)]
    out = host(out)
    if mode == 'colors_u8':                                  # the background colour
      assert (out['rgb'][out['face'] < 0] == np.float32([0.25, 0.5, 0.75])).all()
      out['rgb'][out['face'] < 0] = 1.
    for k in BUFFERS:
      assert np.array_equal(bits(out[k]), bits(ref[k])), (mode, k)
    again = host(ops.raster_shade(dm, P, vis[None], near, **dev_kw))
    assert all(np.array_equal(bits(again[k]), bits(ref[k])) for k in BUFFERS[:5])
  if name == 'hand':
    assert set(np.unique(want['face']).tolist()) <= {-1, 0, 1, 8}                                   # the seven bad faces are never seen
  if name == 'soup' and view != 'near_cut':
    f = want['face']
    assert not ((f >= 50) & (f < 60)).any() and (view == 'inside' or ((f >= 40) & (f < 50)).any())    # of identical faces the lower id
    assert ((f >= 0) & (f < 40)).any() or (f >= 260).any()


def test_render_mesh_is_the_two_calls_and_supersamples():
  m = source('latlong')
  dm = to_device(m)
  eye, target, focal, near = VIEWS['outside']
  ptc, c2w = R.pixtocam(focal, W, H), R.look_at(eye, target)
  want = restated('latlong', 'outside', 'colors_u8')
  r = mesh.render_mesh(dict(dm, colors=torch.from_numpy(np.array(m['colors'])).cuda()), ptc, c2w, H, W, colors=True, near=near)
  assert np.array_equal(r['proj'], projection('outside')[0])
  assert all(np.array_equal(bits(r[k].cpu().numpy()), bits(want[k])) for k in BUFFERS)
  r2 = mesh.render_mesh(dm, None, None, H, W, proj=r['proj'], near=near, texture=dict(texture=torch.from_numpy(np.array(m['texture'])).cuda(),
                                                                                      uv=torch.from_numpy(np.array(m['uv'])).cuda()))
  assert np.array_equal(bits(r2['rgb'].cpu().numpy()), bits(restated('latlong', 'outside', 'texture_u8')['rgb']))
  # supersample 3: the geometric buffers at 3 H x 3 W under diag(3, 3, 1) P, rgb and acc box-averaged
  k = 3
  s = mesh.render_mesh(dm, ptc, c2w, H, W, near=near, supersample=k)
  Pk = np.array(projection('outside')[0])
  Pk[:2] *= np.float32(k)
  assert np.array_equal(s['proj'], Pk)
  fine = R.render(m, Pk, k * H, k * W, near)
  assert tuple(s['face'].shape) == (k * H, k * W) and tuple(s['rgb'].shape) == (H, W, 3) and tuple(s['acc'].shape) == (H, W)
  assert all(np.array_equal(bits(s[n].cpu().numpy()), bits(fine[n])) for n in ('face', 'depth', 'bary', 'normals'))
  acc = fine['acc'].astype(np.float64).reshape(H, k, W, k).mean((1, 3))
  rgb = fine['rgb'].astype(np.float64).reshape(H, k, W, k, 3).mean((1, 3))
  assert np.abs(s['acc'].cpu().numpy() - acc).max() <= 1e-6 and np.abs(s['rgb'].cpu().numpy() - rgb).max() <= 1e-6
  assert ((acc > 0) & (acc < 1)).sum() > 20                   # the silhouette is anti-aliased


# ---- watertightness on the kernels' own cover counts

def kernel_cover_counts(m, P, h, w, near):
  """How many faces cover each pixel, from one single-face visibility buffer per face (test only)."""
  dev = to_device(m)
  counts = torch.zeros((h, w), dtype=torch.int64, device=dev['faces'].device)
  for f in range(len(m['faces'])):
    one = dict(dev, faces=dev['faces'][f:f + 1].contiguous())
    counts += ops.raster_visibility(one, P, h, w, near, check_faces=False) != -1
  return counts.cpu().numpy()


def test_watertight_on_the_kernels_own_cover_counts():
  """120 faces at 32 x 32: from inside every pixel is covered by exactly one face although most faces lie behind or across the
  camera plane; from outside by two or by none.  Precondition (include/mnerf.h, LIMIT): no projected vertex within 1e-3 pixel of a
  pixel centre."""
  m = R.latlong_sphere(6, radius=0.6)
  assert len(m['faces']) == 120
  for view, allowed in (('inside', {1}), ('outside', {0, 2})):
    eye, target, focal, near = VIEWS[view]
    P = mesh.world_to_pixel(R.pixtocam(focal * 32 / 61, 32, 32), R.look_at(eye, target))
    assert R.vertex_clearance(m['vertices'], P) >= 1e-3
    counts = kernel_cover_counts(m, P, 32, 32, near)
    assert set(np.unique(counts).tolist()) == allowed, (view, np.unique(counts, return_counts=True))
    assert np.array_equal(counts, R.visibility(m['vertices'], m['faces'], P, 32, 32, near, counts=True)[1])
  for name in ('latlong', 'sphere'):                          # the full-size inside views: no pixel is left empty
    P, near = projection('inside')
    assert R.vertex_clearance(source(name)['vertices'], P) >= 1e-3
    face = ops.raster_shade(to_device(source(name)), P, ops.raster_visibility(to_device(source(name)), P, H, W, near), near)['face']
    assert bool((face >= 0).all())


# ---- conventions

def conditioning(h, xs, ys, zc):
  """sum_i M_i / S per pixel (float64) for the homogeneous corners h [n,3,3] of the pixels' faces: M_i is the sum of the magnitudes
  that are added and subtracted in E_i, S = |det| / zc.  c * 2^-24 times it bounds the relative rounding error of l_i and zc."""
  p = np.stack([xs + .5, ys + .5, np.ones(len(xs))], -1)
  M = 0.
  for i in range(3):
    a, b = np.abs(h[:, (i + 1) % 3]), np.abs(h[:, (i + 2) % 3])
    M = M + ((a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1]) * p[:, 0] + (a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2]) * p[:, 1] + (a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]))
  return M / (np.abs((np.cross(h[:, 1], h[:, 2]) * h[:, 0]).sum(-1)) / zc)


def test_projection_convention():
  """P (sum l_i X_i, 1) = ((x + .5) zc, (y + .5) zc, zc) for pixel (x, y) with the kernels' bary l and depth zc, in float64 from
  the float32 P and vertices.  Bound, per pixel and row r, from the float32 roundings of the contract: every E_i is a sum of
  products of two h's and a pixel coordinate; with M_i = sum_d (|h_j.a h_k.b| + |h_j.b h_k.a|)_d |p_d| the magnitude of what is added
  and subtracted in E_i, its absolute error is at most c eps M_i with eps = 2^-24 and c = 16 roundings on the way (4 in each h, 1 a
  product, 1 a difference, 2 in the sum, and the relative errors of h enter twice).  l_i = E_i / S and zc = |det| / S inherit it
  relative to S, so row r is off by at most  c eps (sum_i M_i / S) (max_i |h_i[r]| + |target_r|) + c eps |target_r|."""
  for name, view in (('latlong', 'outside'), ('latlong', 'inside'), ('sphere', 'outside')):
    m = source(name)
    P, near = projection(view)
    out = host(ops.raster_shade(to_device(m), P, ops.raster_visibility(to_device(m), P, H, W, near), near))
    ys, xs = np.nonzero(out['face'] >= 0)
    ids = m['faces'][out['face'][ys, xs]]
    X = m['vertices'].astype(np.float64)[ids]                                                       # [n,3,3]
    l, zc = out['bary'][ys, xs].astype(np.float64), out['depth'][ys, xs].astype(np.float64)
    P64 = P.astype(np.float64)
    q = (l[:, :, None] * X).sum(1) @ P64[:, :3].T + P64[:, 3]
    target = np.stack([(xs + .5) * zc, (ys + .5) * zc, zc], -1)
    h = X @ P64[:, :3].T + P64[:, 3]                                                                # [n,corner,3]
    MS = conditioning(h, xs, ys, zc)
    eps, c = 2.0 ** -24, 16.
    bound = c * eps * MS[:, None] * (np.abs(h).max(1) + np.abs(target)) + c * eps * np.abs(target)
    ratio = (np.abs(q - target) / bound).max()
    print(f'{name} {view}: {len(ys)} pixels, max |P X - target| {np.abs(q - target).max():.3e}, largest error / bound {ratio:.3f}')
    assert ratio <= 1.


def test_front_is_pinned():
  """`front`: counter-clockwise seen from the camera, which under world_to_pixel's flip of y is det < 0.  A sphere whose faces are
  counter-clockwise seen from outside (positive signed volume) looks the same from outside with cull = 'back' as without, and from
  inside nothing of it is left."""
  for name in ('latlong', 'sphere'):
    m = source(name)
    assert mesh.mesh_stats(m['vertices'], m['faces'])['signed_volume'] > 0
    dm = to_device(m)
    P, near = projection('outside')
    both, back = (ops.raster_visibility(dm, P, H, W, near, cull=c) for c in ('none', 'back'))
    assert torch.equal(both, back) and int((both != -1).sum()) > 200
    su = R.setup(m['vertices'], m['faces'], P)
    assert (su['s'][host(ops.raster_shade(dm, P, both, near))['face'][both.cpu().numpy() != -1]] == -1).all()
    P, near = projection('inside')
    assert bool((ops.raster_visibility(dm, P, H, W, near, cull='back') == -1).all())
    r = mesh.render_mesh(dm, None, None, H, W, proj=P, near=near, cull='back', bg=(0., 0.5, 1.))
    assert bool((r['face'] == -1).all()) and bool((r['acc'] == 0).all()) and bool((r['rgb'] == torch.tensor([0., 0.5, 1.]).cuda()).all())
    flipped = dict(dm, faces=dm['faces'][:, [0, 2, 1]].contiguous())
    assert bool((ops.raster_visibility(flipped, P, H, W, near, cull='back') != -1).all())


# ---- the analytic dataset

def inscribed_radius(m):
  """The distance from the origin to the nearest point of the mesh, float64 (vertices on the unit sphere: the nearest point of a face
  is the foot of the perpendicular where that lies inside the face, else the midpoint of an edge)."""
  v = m['vertices'].astype(np.float64)[m['faces']]
  n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
  n /= np.linalg.norm(n, axis=-1, keepdims=True)
  d = (n * v[:, 0]).sum(-1)
  foot = d[:, None] * n
  inside = np.ones(len(v), bool)
  for i in range(3):
    inside &= (np.cross(v[:, (i + 1) % 3] - v[:, i], foot - v[:, i]) * n).sum(-1) >= 0
  mid = np.stack([np.linalg.norm((v[:, i] + v[:, (i + 1) % 3]) / 2, axis=-1) for i in range(3)], -1).min(-1)
  return float(np.where(inside, np.abs(d), mid).min())


@functools.lru_cache(maxsize=None)
def procedural(split):
  from multinerf_amd import configs, datasets
  config = configs.load_preset('blender_256', ["Config.dataset_loader = 'procedural'", 'Config.factor = 2'])
  return config, datasets.load_dataset(split, config.data_dir, config, device='cuda')


def unit_sphere():
  m = R.latlong_sphere(24)
  m['vertices'] = (m['vertices'].astype(np.float64) / np.linalg.norm(m['vertices'].astype(np.float64), axis=-1, keepdims=True)).astype(np.float32)
  return m


def test_against_the_analytic_sphere_of_the_procedural_dataset():
  """The `procedural` test cameras at 48 x 48 and a sphere mesh with its vertices on the unit sphere (inscribed radius r_in, float64):
  a pixel whose ray (the dataset's own, camera_utils.pixels_to_rays) hits the ball of radius r_in must be covered, one whose ray
  misses the unit ball must not be, and a covered pixel's surface point p_hit = sum l_i X_i lies within 1 - r_in of the unit sphere.
  The point o + depth d along the ray is held to the same bound plus the float32 rounding of depth = |det| / S: taken literally it
  misses on two of the six views (MI355X), view 0 with 4.268708e-03 and view 5 with 4.338286e-03 against 1 - r_in = 4.268482e-03,
  by 2.3e-07 and 7.0e-05; the latter is 2e-5 of a depth near 3.5, the cancellation in det and S that tests/test_raster_cpu.py
  measures (7e-5 relative), at a pixel whose ray meets a face near its deepest point."""
  config, dataset = procedural('test')
  assert (dataset.height, dataset.width) == (48, 48)
  m = unit_sphere()
  r_in = inscribed_radius(m)
  assert 0.98 < r_in < 1.
  dm = to_device(m)
  for idx in range(dataset.size):
    r = mesh.render_mesh(dm, dataset.pixtocams, dataset.camtoworlds[idx], 48, 48, near=config.near)
    rays = dataset.generate_ray_batch(idx).rays
    o, d = rays.origins.cpu().numpy().astype(np.float64), rays.directions.cpu().numpy().astype(np.float64)
    acc, depth = r['acc'].cpu().numpy(), r['depth'].cpu().numpy().astype(np.float64)
    a, b, cc = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1)
    hits = lambda radius: b * b - a * (cc - radius * radius) > 0
    assert (acc[hits(r_in)] == 1).all() and (acc[~hits(1.)] == 0).all()
    assert hits(r_in).sum() > 300 and (~hits(1.)).sum() > 300
    v = m['vertices'].astype(np.float64)[m['faces'][np.maximum(r['face'].cpu().numpy(), 0)]]               # [48,48,corner,3]
    p = (r['bary'].cpu().numpy().astype(np.float64)[..., None] * v).sum(-2)
    off = np.abs(np.linalg.norm(p, axis=-1) - 1.)[acc == 1]
    assert off.max() <= 1 - r_in
    # the same point along the ray, o + depth d: depth carries the float32 rounding of |det| / S, at most 16 * 2^-24 * (sum_i M_i / S)
    # of itself (test_projection_convention derives it), which a point that lies r_in deep to begin with does not have to spare
    ys, xs = np.nonzero(acc == 1)
    P64 = r['proj'].astype(np.float64)
    allowance = 16 * 2.0 ** -24 * conditioning(v[ys, xs] @ P64[:, :3].T + P64[:, 3], xs, ys, depth[ys, xs]) * depth[ys, xs] * np.linalg.norm(d[ys, xs], axis=-1)
    ray = np.abs(np.linalg.norm(o[ys, xs] + depth[ys, xs, None] * d[ys, xs], axis=-1) - 1.)
    print(f'view {idx}: {int(acc.sum())} covered, {int((hits(1.) & ~hits(r_in)).sum())} free, max ||p| - 1| {off.max():.6e} (along the ray '
          f'{ray.max():.6e}, rounding allowance up to {allowance.max():.1e}) of {1 - r_in:.6e}')
    assert (ray <= 1 - r_in + allowance).all()


# ---- the atlas's seam claim, by rendering

def linear_colour(p):
  return 0.5 + 0.2 * p[..., [0, 1, 2]] + 0.1 * p[..., [1, 2, 0]]


def chart_offset(face, cols):
  """0 .. 28 in steps of 4, different for any two faces whose charts touch (the same cell, or cells that are neighbours along a row,
  a column or a diagonal of the atlas)."""
  cell = face // 2
  return 4. * (face % 2) + 8. * ((cell % cols) % 2) + 16. * ((cell // cols) % 2)


@pytest.mark.parametrize('c', (3, 8))
def test_the_atlas_is_seam_free_when_rendered(c):
  """The atlas's claim, a bilinear lookup inside a face's UV triangle never reads a neighbour's texel, checked by rendering.  The atlas
  (cell c, point samples; bake_texture's own three steps, ops.atlas_samples / atlas_store / atlas_uvs, so that the colour can depend
  on the owning face) holds  t = a g(p) + b off(f)  with g(p) = 0.5 + 0.2 p + 0.1 perm(p) LINEAR in position and off(f) a
  far-away constant per chart, at least 4 apart between any two charts that touch.  Rendered, rgb must be a g(p_hit) + b off(face)
  with p_hit = sum l_i X_i: reading a neighbour's texel with weight w would be off by at least 4 b w.

  Bound.  Bilinear interpolation of a function that is linear over a face's own texels is exact in exact arithmetic.  In float32:
  (1) the lookup position: uv is stored rounded (2^-24, the leak the atlas tests measured), its blend rounds three times, sum l_i
  is 1 to 2^-23 only, and x = u Wt - .5 rounds once more: 7 * 2^-24 * max(Wt, Ht) =: delta texels, along each axis.  That shifts the
  lookup inside the chart, a G a texel with G = max_edges |g(v_j) - g(v_k)| / (c - 2), and it leaks a weight delta onto a texel of
  another chart, up to D = 28 b + 0.4 a + a G away;  (2) a texel is a float32: 2^-24 Tmax, and the blend rounds 6 times: 8 * 2^-24
  Tmax with Tmax = a + 28 b;  (3) the constant 0.5 a is scaled by sum l_i: 2^-22.
    |rgb - expected| <= 2 delta (a G + D) + 8 * 2^-24 Tmax + 2^-22.
  float32 atlas, a = b = 1, c = 8 (612 x 616 texels): 0.015, where one leaked texel at weight 1/2 is 2 (measured: 3.8e-6).  The uint8
  atlas (a = 0.25, b = 0.025, values below 0.95) adds its quantisation 1 / 510: 2.4e-3, where one leaked texel at weight 1/2 is 0.05
  (measured: 1.9e-3, the quantisation)."""
  m = source('sphere')
  dm = to_device(m)
  T = len(m['faces'])
  lay = ops.atlas_layout(T, c)
  Ht, Wt, n = lay['H'], lay['W'], lay['n_samples']
  means, _, _, _, owner = ops.atlas_samples(dm, lay, 0, n, filter=0.)
  uv = ops.atlas_uvs(dm, lay)
  g = linear_colour(means.cpu().numpy().astype(np.float64))
  off = chart_offset(np.maximum(owner.cpu().numpy().astype(np.int64), 0), lay['cols'])[:, None]
  v = m['vertices'].astype(np.float64)[m['faces']]
  gv = linear_colour(v)
  G = max(np.abs(gv[:, j] - gv[:, k]).max() for j, k in ((0, 1), (1, 2), (2, 0))) / (c - 2)
  eps = 2.0 ** -24
  delta = 7 * eps * max(Wt, Ht)
  for a, b, key in ((1., 1., 'f32'), (0.25, 0.025, 'u8')):
    texture = torch.zeros((Ht, Wt, 3), dtype=torch.uint8).cuda()
    mask = torch.zeros((Ht, Wt), dtype=torch.uint8).cuda()
    texture_f32 = torch.zeros((Ht, Wt, 3), dtype=torch.float32).cuda()
    rgb = torch.from_numpy(np.ascontiguousarray(a * g + b * off, dtype=np.float32)).cuda()
    ops.atlas_store(dm, lay, 0, rgb, owner, texture, mask, texture_f32)
    bound = 2 * delta * (a * G + 28 * b + 0.4 * a + a * G) + 8 * eps * (a + 28 * b) + 2.0 ** -22 + (1. / 510. if key == 'u8' else 0.)
    for view in ('outside', 'inside'):
      P, near = projection(view)
      r = host(mesh.render_mesh(dm, None, None, H, W, proj=P, near=near, texture=dict(texture=texture_f32 if key == 'f32' else texture, uv=uv)))
      ys, xs = np.nonzero(r['face'] >= 0)
      f = r['face'][ys, xs].astype(np.int64)
      p = (r['bary'][ys, xs].astype(np.float64)[:, :, None] * v[f]).sum(1)
      err = np.abs(r['rgb'][ys, xs] - (a * linear_colour(p) + b * chart_offset(f, lay['cols'])[:, None])).max()
      print(f'c {c} {view} {key}: atlas {Wt} x {Ht}, {len(ys)} pixels, max |rgb - expected| {err:.3e}, bound {bound:.3e}, a leaked texel at 1/2: {2 * b}')
      assert len(ys) > 200 and err <= bound < 0.1 * 2 * b


# ---- TSDF round trip

def test_tsdf_round_trip():
  """depth / acc of a unit-sphere mesh from the procedural train cameras, fused by TsdfVolume and meshed again: the new vertices lie
  within one grid spacing plus 1 - r_in of the unit sphere.  A depth that were the ray's length instead of zc, or half a pixel off,
  would not."""
  config, dataset = procedural('train')
  m = unit_sphere()
  r_in = inscribed_radius(m)
  dm = to_device(m)
  volume = mesh.TsdfVolume((-1.25,) * 3, (1.25,) * 3, 33, colors=False)
  for idx in range(0, dataset.size, 2):
    r = mesh.render_mesh(dm, dataset.pixtocams, dataset.camtoworlds[idx], dataset.height, dataset.width, near=config.near)
    volume.integrate(r['depth'], torch.from_numpy(r['proj']).cuda(), acc=r['acc'])
  out = volume.mesh()
  radius = np.linalg.norm(out['vertices'].cpu().numpy().astype(np.float64), axis=-1)
  print(f'{len(radius)} vertices, | |v| - 1 | max {np.abs(radius - 1).max():.4f}, allowed {volume.spacing + 1 - r_in:.4f}')
  assert len(radius) > 1000 and np.abs(radius - 1).max() <= volume.spacing + (1 - r_in)


# ---- argument checks and degenerate inputs

def test_argument_checks():
  m = source('latlong')
  dm = to_device(m)
  P, near = projection('outside')
  ok = ops.raster_visibility(dm, P, H, W, near)
  cpu = {k: v.cpu() for k, v in dm.items()}
  bad_index = dict(dm, faces=dm['faces'].clone())
  bad_index['faces'][3, 1] = len(m['vertices'])
  cases = [
      lambda: ops.raster_visibility(dict(dm, faces=dm['faces'].long()), P, H, W, near),
      lambda: ops.raster_visibility(dict(dm, vertices=dm['vertices'].double()), P, H, W, near),
      lambda: ops.raster_visibility(dict(dm, normals=dm['normals'][:-1]), P, H, W, near),
      lambda: ops.raster_visibility(dict(dm, faces=dm['faces'].reshape(-1, 2)), P, H, W, near),
      lambda: ops.raster_visibility(bad_index, P, H, W, near),
      lambda: ops.raster_visibility(dm, P, H, W, 0.),
      lambda: ops.raster_visibility(dm, P, H, W, -1.),
      lambda: ops.raster_visibility(dm, P, H, W, float('inf')),
      lambda: ops.raster_visibility(dm, P, H, W, float('nan')),
      lambda: ops.raster_visibility(dm, P, 0, W, near),
      lambda: ops.raster_visibility(dm, P, H, 0, near),
      lambda: ops.raster_visibility(dm, P[:2], H, W, near),
      lambda: ops.raster_visibility(dm, P * np.float32('nan'), H, W, near),
      lambda: ops.raster_visibility(dm, P, H, W, near, cull='front'),
      lambda: ops.raster_visibility(dm, P, H, W, near, threshold=-1),
      lambda: ops.raster_shade(dm, P, ok.int(), near),
      lambda: ops.raster_shade(dm, P, ok[0], near),
      lambda: ops.raster_shade(dm, P, ok, near, colors=torch.zeros((5, 3), dtype=torch.uint8).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, colors=torch.zeros((len(m['vertices']), 3), dtype=torch.float64).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, texture=torch.zeros((4, 4, 3)).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, texture=torch.zeros((4, 4, 3)).cuda(), uv=torch.zeros((7, 3, 2)).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, texture=torch.zeros((4, 4)).cuda(), uv=torch.zeros((len(m['faces']), 3, 2)).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, uv=torch.zeros((len(m['faces']), 3, 2)).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, colors=torch.zeros((len(m['vertices']), 3)).cuda(), texture=torch.zeros((4, 4, 3)).cuda(),
                               uv=torch.zeros((len(m['faces']), 3, 2)).cuda()),
      lambda: ops.raster_shade(dm, P, ok, near, bg=(1., 1.)),
      lambda: mesh.render_mesh(dm, None, None, H, W, proj=P, supersample=0),
      lambda: mesh.render_mesh(dm, None, None, 0, W, proj=P),
      lambda: mesh.render_mesh(dm, R.pixtocam(50., W, H), R.look_at((2., 1., 1.)), H, W, cull='front'),
  ]
  if os.environ.get('MNR_TESTS_ON_SIMULATOR') != '1':       # (on the simulator every tensor is a host tensor)
    cases.append(lambda: ops.raster_visibility(cpu, P, H, W, near))
  for n, case in enumerate(cases):
    with pytest.raises(ValueError):
      case()
      print('case', n, 'did not raise')
  from multinerf_amd import camera_utils
  with pytest.raises(ValueError, match='fisheye'):
    mesh.world_to_pixel(R.pixtocam(50., W, H), R.look_at((2., 1., 1.)), camtype=camera_utils.ProjectionType.FISHEYE)
  assert torch.equal(ops.raster_visibility(dm, P, H, W, near), ok)          # and nothing was disturbed


def test_degenerate_inputs():
  m = source('latlong')
  dm = to_device(m)
  P, near = projection('outside')
  empty = lambda r, h=H, w=W: (tuple(r['face'].shape) == (h, w) and bool((r['face'] == -1).all()) and bool((r['acc'] == 0).all()) and
                               bool((r['depth'] == 0).all()) and bool((r['bary'] == 0).all()) and bool((r['normals'] == 0).all()) and
                               bool((r['rgb'] == torch.tensor([0.1, 0.2, 0.3]).cuda()).all()))
  bg = (0.1, 0.2, 0.3)
  # a mesh without faces, with and without vertices
  none = dict(dm, faces=torch.zeros((0, 3), dtype=torch.int32).cuda())
  assert empty(mesh.render_mesh(none, None, None, H, W, proj=P, near=near, bg=bg))
  nothing = dict(vertices=torch.zeros((0, 3)).cuda(), normals=torch.zeros((0, 3)).cuda(), faces=none['faces'])
  assert empty(mesh.render_mesh(nothing, None, None, H, W, proj=P, near=near, bg=bg))
  assert bool((ops.raster_visibility(none, P, H, W, near) == -1).all())
  assert empty(ops.raster_shade(none, P, ops.raster_visibility(none, P, H, W, near), near, bg=bg))
  # a mesh entirely behind the camera: look the other way
  eye, target, focal, _ = VIEWS['outside']
  away = mesh.world_to_pixel(R.pixtocam(focal, W, H), R.look_at(eye, tuple(2 * np.array(eye))))
  assert (R.homogeneous(m['vertices'], away)[:, 2] < 0).all()
  assert empty(mesh.render_mesh(dm, None, None, H, W, proj=away, near=near, bg=bg))
  assert empty(mesh.render_mesh(dm, None, None, H, W, proj=away, near=near, bg=bg, threshold=0))
  # near beyond everything
  assert empty(mesh.render_mesh(dm, None, None, H, W, proj=P, near=10., bg=bg))
  # a 1 x 1 image, centred on the sphere, and a supersampled one
  one = mesh.world_to_pixel(R.pixtocam(5., 1, 1), R.look_at(eye, (0., 0., 0.)))
  r = mesh.render_mesh(dm, None, None, 1, 1, proj=one, near=near, bg=bg)
  want = R.render(m, one, 1, 1, near)
  assert tuple(r['rgb'].shape) == (1, 1, 3) and int(r['face'][0, 0]) == int(want['face'][0, 0]) >= 0
  assert np.array_equal(bits(r['depth'].cpu().numpy()), bits(want['depth'])) and abs(float(r['depth'][0, 0]) - (np.linalg.norm(eye) - 0.6)) < 0.01
  r = mesh.render_mesh(dm, None, None, 1, 1, proj=one, near=near, bg=bg, supersample=4)
  assert tuple(r['rgb'].shape) == (1, 1, 3) and tuple(r['face'].shape) == (4, 4)


# ---- eval_mesh.py

def procedural_shading(p):
  """The dataset's own shading of a point of the unit sphere (datasets.Procedural)."""
  n = p / np.maximum(np.linalg.norm(p, axis=-1, keepdims=True), 1e-9)
  light = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
  return (0.5 + 0.5 * n) * (0.3 + 0.7 * np.clip(n @ light, 0, 1)[..., None])


def psnr_of(rgb, gt):
  q = np.rint(np.clip(rgb.astype(np.float64), 0, 1) * 255.) / 255.
  return -10. * np.log10(((q - gt.astype(np.float64)) ** 2).mean())


def run_eval(args):
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'eval_mesh.py')] + args, capture_output=True, text=True,
                     env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
  print(r.stdout[-3000:], r.stderr[-3000:])
  assert r.returncode == 0
  return r.stdout


def test_eval_mesh_script(tmp_path):
  """eval_mesh.py on the procedural preset at factor 2 (six 48 x 48 test views): a sphere coloured per vertex with the dataset's own
  shading, then the same with a baked texture (the PNG path).  Every view's PSNR is the PSNR of the restatement's rendering of that
  view to 1e-3 dB; the values are recorded in profiles/mesh_render.md."""
  config, dataset = procedural('test')
  m = unit_sphere()
  m['colors'] = np.floor(np.clip(procedural_shading(m['vertices'].astype(np.float64)), 0, 1) * 255 + 0.5).astype(np.uint8)
  binds = ['--preset', 'blender_256', '--gin_bindings', "Config.dataset_loader = 'procedural'", '--gin_bindings', 'Config.factor = 2']
  gts = np.asarray(torch.as_tensor(dataset.images).cpu().numpy(), np.float64)[..., :3]
  projs = [mesh.world_to_pixel(dataset.pixtocams, dataset.camtoworlds[i]) for i in range(dataset.size)]

  def check(out_dir, **colour):
    for name in ('mesh_metric_psnr.txt', 'mesh_metric_ssim.txt', 'mesh_render_times.txt'):
      assert os.path.exists(os.path.join(out_dir, name)), name
    psnrs = [float(v) for v in open(os.path.join(out_dir, 'mesh_metric_psnr.txt')).read().split()]
    ssims = [float(v) for v in open(os.path.join(out_dir, 'mesh_metric_ssim.txt')).read().split()]
    assert len(psnrs) == len(ssims) == dataset.size == 6 and all(0.5 < s <= 1. for s in ssims)
    from PIL import Image
    for i in range(dataset.size):
      want = R.render(m, projs[i], 48, 48, config.near, **colour)
      ref = psnr_of(want['rgb'], gts[i])
      print(f'view {i}: psnr {psnrs[i]:.4f}, restatement {ref:.4f}, ssim {ssims[i]:.4f}')
      assert abs(psnrs[i] - ref) <= 1e-3
      png = np.asarray(Image.open(os.path.join(out_dir, f'mesh_color_{i:03d}.png')))
      assert png.shape == (48, 48, 3) and np.array_equal(png, np.rint(np.clip(want['rgb'].astype(np.float64), 0, 1) * 255).astype(np.uint8))
    return psnrs

  ply = str(tmp_path / 'sphere.ply')
  mesh.write_ply(ply, m)
  run_eval(['--mesh', ply] + binds)
  check(str(tmp_path / 'mesh_eval'), colors=m['colors'])
  # textured: bake the same function, write PLY + PNG, read them back as the script does
  dm = to_device(m)
  baked = mesh.bake_texture(dm, color_fn=lambda means, covs, normals, viewdirs: torch.from_numpy(
      procedural_shading(means.cpu().numpy().astype(np.float64))).to(device=means.device, dtype=torch.float32), cell=6, filter=0.)
  ply = str(tmp_path / 'textured.ply')
  mesh.write_ply(ply, {k: m[k] for k in ('vertices', 'normals', 'faces')}, texture=baked)
  out_dir = str(tmp_path / 'textured_eval')
  run_eval(['--mesh', ply, '--out_dir', out_dir, '--supersample', '1', '--cull', 'back'] + binds)
  back = mesh.read_ply(ply)
  check(out_dir, texture=baked['texture'].cpu().numpy(), uv=back['texcoord'])
