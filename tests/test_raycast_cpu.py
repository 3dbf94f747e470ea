"""The NumPy restatement of csrc/meshray.hip (tests/raycast_ref.py) held against answers that are known: a unit triangle, shared edges
and a shared vertex of a closed fan, parallel and behind-origin rays, the two ends of (t_min, t_max], both windings under cull, faces
without area, directions with zero components, rays that are not finite, an independent float64 Moller-Trumbore brute force on a
generic soup, and the rasteriser's restatement on one view.  tests/test_gpu_raycast.py holds the kernels to the restatement bit for
bit; this file is what makes that mean something."""

import functools

import numpy as np

from tests import raster_ref as R
from tests import raycast_ref as Q
from tests.test_gpu_raster import H, VIEWS, W, projection

F = np.float32
U24 = 2.0 ** -24
INF = np.float32('inf')

TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
TRI_F = np.array([[0, 1, 2]], np.int32)


def one(o, d, verts=TRI_V, faces=TRI_F, **kw):
  t, f, b = Q.cast(np.array([o], F), np.array([d], F), verts, faces, **kw)
  return float(t[0]), int(f[0]), b[0]


def missed(r):
  return r[0] == np.inf and r[1] == -1 and (r[2] == 0).all()


def test_unit_triangle_known_answer():
  t, f, b = one((0.25, 0.25, 1.), (0., 0., -1.))
  assert (t, f) == (1., 0) and np.array_equal(b, F([0.5, 0.25, 0.25]))
  t, f, b = one((0.25, 0.25, 1.), (0., 0., -2.))              # t is in units of |d|
  assert (t, f) == (0.5, 0) and np.array_equal(b, F([0.5, 0.25, 0.25]))
  t, f, b = one((0.125, 0.5, -3.), (0., 0., 4.))              # from the other side
  assert (t, f) == (0.75, 0) and np.array_equal(b, F([0.375, 0.125, 0.5]))
  t, f, b = one((1.25, 0.25, 1.), (-1., 0., -1.))              # oblique: the point (0.25, 0.25, 0)
  assert (t, f) == (1., 0) and np.array_equal(b, F([0.5, 0.25, 0.25]))
  assert missed(one((0.75, 0.75, 1.), (0., 0., -1.)))        # beside it


def test_parallel_and_behind_origin_rays_miss():
  assert missed(one((0.25, 0.25, 1.), (1., 0., 0.)))          # parallel to the plane, above it
  assert missed(one((-1., 0.25, 0.), (1., 0., 0.)))           # IN the plane: edge-on, det = 0
  assert missed(one((0.25, 0.25, 1.), (0., 0., 1.)))          # the face lies behind the origin
  assert missed(one((0.25, 0.25, 0.), (0., 0., 1.)))          # the origin ON the face: t = 0 is not > t_min = 0


def test_t_min_is_exclusive_and_t_max_inclusive():
  o, d = (0.25, 0.25, 1.), (0., 0., -1.)
  assert one(o, d, t_min=0.5, t_max=1.)[:2] == (1., 0)
  assert missed(one(o, d, t_min=1.))
  assert one(o, d, t_min=float(np.nextafter(F(1), F(0))))[:2] == (1., 0)
  assert missed(one(o, d, t_max=float(np.nextafter(F(1), F(0)))))
  assert one(o, d, t_max=np.inf)[:2] == (1., 0)
  two = np.concatenate([TRI_V, TRI_V + F([0, 0, -1])])        # a second face one unit behind: t_min skips the first
  faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
  assert one(o, d, two, faces)[:2] == (1., 0) and one(o, d, two, faces, t_min=1.)[:2] == (2., 1)
  assert missed(one(o, d, two, faces, t_min=1., t_max=1.5))


def test_both_windings_with_cull():
  """Front is counter-clockwise seen from the ray origin: the geometric normal (b - a) x (c - a) has a negative product with d."""
  flipped = TRI_F[:, ::-1].copy()
  above, below = ((0.25, 0.25, 1.), (0., 0., -1.)), ((0.25, 0.25, -1.), (0., 0., 1.))      # the normal of TRI is +z
  for (o, d), faces, front in ((above, TRI_F, True), (below, TRI_F, False), (above, flipped, False), (below, flipped, True)):
    assert one(o, d, faces=faces)[:2] == (1., 0)
    assert (one(o, d, faces=faces, cull='back')[:2] == (1., 0)) == front and missed(one(o, d, faces=faces, cull='back')) != front
  # every axis and sign as the dominant one, on a generic soup: cull = 'back' keeps exactly the hits whose float64 normal faces the ray
  m = generic_soup()
  o, d = soup_rays()
  v = m['vertices'].astype(np.float64)[m['faces']]
  n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
  h = Q.hits(o[:400], d[:400], m['vertices'], m['faces'])
  hb = Q.hits(o[:400], d[:400], m['vertices'], m['faces'], cull='back')
  facing = (d[:400].astype(np.float64)[:, None, :] * n[None]).sum(-1) < 0
  assert h['eligible'].sum() > 1000 and np.array_equal(hb['eligible'], h['eligible'] & facing)
  assert len(set(zip(*[Q.shear(o[:400], d[:400])[k].tolist() for k in ('kx', 'ky', 'kz')]))) == 6


def test_faces_without_area_are_never_hit():
  v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [0.25, 0.125, 0.5], [0.5, 0.25, 1.], [1., 0.5, 2.]], F)
  faces = np.array([[0, 1, 1], [1, 1, 1], [1, 2, 3], [4, 5, 6], [0, 2, 2]], np.int32)      # two equal, three equal, collinear, collinear, two equal
  rng = np.random.default_rng(3)
  o = rng.uniform(-2, 2, (3000, 3)).astype(F)
  # aimed at points of the segments the faces degenerate to, at their corners, and anywhere
  s = rng.uniform(0, 1, (3000, 1)).astype(F)
  seg = [(0, 1), (1, 1), (1, 2), (4, 6), (0, 2)]
  ends = np.array([seg[i % 5] for i in range(3000)])
  target = v[ends[:, 0]] + s * (v[ends[:, 1]] - v[ends[:, 0]])
  target[::7] = v[ends[::7, 0]]
  d = (target - o).astype(F)
  d[1::3] = rng.normal(size=(1000, 3)).astype(F)
  t, f, b, det = Q.cast(o, d, v, faces, details=True)
  assert (f == -1).all() and (t == np.inf).all() and (b == 0).all() and (det['count'] == 0).all()


def test_directions_with_zero_components():
  v = np.array([[-1, -1, 0.5], [2, -1, 0.5], [-1, 2, 0.5], [0.5, -1, -1], [0.5, 2, -1], [0.5, -1, 2]], F)
  faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)          # the planes z = 0.5 and x = 0.5
  cases = [((0.25, 0.25, 0.), (0., 0., 1.), 0.5, 0), ((0.25, 0.25, 2.), (0., 0., -0.5), 3., 0), ((0., 0.25, 0.25), (1., 0., 0.), 0.5, 1),
           ((2., 0.25, 0.25), (-3., 0., 0.), 0.5, 1), ((0., 0., 0.), (0., 1., 1.), 0.5, 0), ((0., 0., 0.25), (1., 1., 0.), 0.5, 1),
           ((0., 0., 0.), (1., 0., 1.), 0.5, 0), ((0., 0.25, 0.), (-0., 0., 1.), 0.5, 0)]
  for o, d, t, f in cases:
    got = one(o, d, v, faces)
    assert got[:2] == (t, f), (o, d, got)
  assert missed(one((0.25, 0.25, 0.), (0., 1., 0.), v, faces)) and missed(one((0., 0., 0.), (0., -1., 0.), v, faces))
  # equal magnitudes: the dominant axis is the lowest index
  sh = Q.shear(np.zeros((4, 3), F), F([[1, 1, 1], [0, -2, 2], [-3, 0, 3], [1, -1, 0]]))
  assert sh['kz'].tolist() == [0, 1, 0, 0] and sh['kx'].tolist() == [1, 0, 2, 1] and sh['ky'].tolist() == [2, 2, 1, 2]


def test_rays_that_are_not_finite_get_the_empty_result():
  nan = np.nan
  for o, d in (((nan, 0.25, 1.), (0., 0., -1.)), ((0.25, 0.25, np.inf), (0., 0., -1.)), ((0.25, 0.25, 1.), (0., nan, -1.)),
               ((0.25, 0.25, 1.), (0., 0., -np.inf)), ((0.25, 0.25, 1.), (0., 0., 0.)), ((0.25, 0.25, 1.), (0., 0., -1e-45)),
               ((0.25, 0.25, 1.), (np.inf, 0., -1.))):
    assert missed(one(o, d)), (o, d)
  # a face that is not valid is never hit; its neighbour is
  v = np.concatenate([TRI_V, [[nan, 0, 0]]]).astype(F)
  for bad in ([0, 1, 3], [0, 1, 4], [-1, 1, 2]):
    assert missed(one((0.25, 0.25, 1.), (0., 0., -1.), v, np.array([bad], np.int32)))
    assert one((0.25, 0.25, 1.), (0., 0., -1.), v, np.array([bad, [0, 1, 2]], np.int32))[:2] == (1., 1)
  t, f, b = Q.cast(np.zeros((0, 3), F), np.zeros((0, 3), F), TRI_V, TRI_F)
  assert t.shape == (0,) and f.shape == (0,) and b.shape == (0, 3)
  assert missed(one((0.25, 0.25, 1.), (0., 0., -1.), TRI_V, np.zeros((0, 3), np.int32)))


# ---- shared edges and a shared vertex

def fan(n=7, seed=11):
  """A closed fan: n faces around vertex 0 (a cone with a ragged rim), counter-clockwise seen from +z."""
  rng = np.random.default_rng(seed)
  ang = np.sort(rng.uniform(0, 2 * np.pi, n))
  rim = np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.3, 0.3, n)], -1) * rng.uniform(0.7, 1.3, (n, 1))
  v = np.concatenate([[[0.013, -0.021, 0.4]], rim]).astype(F)
  return v, np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)


def test_shared_edges_and_the_shared_vertex_are_never_missed():
  """Rays aimed (to float32 rounding) at points of the fan's inner edges and at its centre vertex, from origins on either side: every
  one hits (a shared edge is hit by both faces or by one, never by neither), and the winner is the lowest key among the faces the
  ray passes.  Exactly representable cases: both faces of an edge and all faces at the vertex pass with equal t, and the lowest id wins."""
  v, faces = fan()
  rng = np.random.default_rng(12)
  n = 4000
  o = (rng.uniform(-0.2, 0.2, (n, 3)) + [0, 0, 3.]).astype(F)       # near the axis: no spoke is a silhouette edge from there
  o[::2, 2] *= -1
  spoke = rng.integers(1, len(v), n)
  s = rng.uniform(0.02, 0.9, (n, 1)).astype(F)
  target = v[0] + s * (v[spoke] - v[0])
  target[::5] = v[0]
  d = ((target - o) * rng.choice([0.001, 1., 1000.], (n, 1))).astype(F)
  t, f, b, det = Q.cast(o, d, v, faces, details=True)
  assert (f >= 0).all() and np.isfinite(t).all() and (det['count'] >= 1).all()
  assert (det['count'][::5] >= 2).sum() > 100 and (det['count'] >= 2).sum() > 300      # the ties do occur
  on_edge = (f[np.arange(n) % 5 != 0] == spoke[np.arange(n) % 5 != 0] - 1) | ((f[np.arange(n) % 5 != 0] + 1) % len(faces) == spoke[np.arange(n) % 5 != 0] - 1)
  assert on_edge.all()                                        # the winner is one of the two faces of the spoke
  # exact: a flat fan in z = 0 around the origin, rays straight down onto an edge midpoint and onto the vertex
  flat = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], F)
  ff = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], np.int32)
  t, f, b, det = Q.cast(F([[0, 0.5, 2], [0, 0, 2], [-0.5, 0, 2]]), F([[0, 0, -1]] * 3), flat, ff, details=True)
  assert t.tolist() == [2., 2., 2.] and f.tolist() == [0, 0, 1] and det['count'].tolist() == [2, 4, 2]
  assert np.array_equal(b, F([[0.5, 0, 0.5], [1, 0, 0], [0.5, 0, 0.5]]))


# ---- an independent float64 brute force

SOUP_SEED = 5
# the worst |t - t_64| / t_64 of the restatement against float64 Moller-Trumbore over the unambiguous rays of the set below, measured on
# the CPU (also in profiles/mesh_raycast.md); the test holds t to 8 times this
MEASURED_T_DEVIATION = 1.591e-4


@functools.lru_cache(maxsize=None)
def generic_soup(T=300, seed=SOUP_SEED):
  rng = np.random.default_rng(seed)
  return dict(vertices=rng.uniform(-0.6, 0.6, (3 * T, 3)).astype(F), faces=np.arange(3 * T, dtype=np.int32).reshape(T, 3))


@functools.lru_cache(maxsize=None)
def soup_rays(n=2000, seed=SOUP_SEED):
  rng = np.random.default_rng(seed + 1)
  o = rng.uniform(-0.7, 0.7, (n, 3))
  o[n // 2:] = 3. * rng.normal(size=(n - n // 2, 3))
  target = rng.uniform(-0.5, 0.5, (n, 3))
  target[::4] = rng.uniform(-1.5, 1.5, (len(target[::4]), 3))        # a quarter aimed more widely: the misses
  d = (target - o) * rng.uniform(0.2, 5., (n, 1))
  return o.astype(F), d.astype(F)


def test_against_float64_moller_trumbore_on_a_generic_soup():
  """300 generic faces x 2000 rays.  A ray is AMBIGUOUS, and left out, when the float64 reference has a candidate hit (a face with
  t > 0 that is not behind the nearest clear hit) with a barycentric within 1e-4 of 0, or its two nearest hits within 1e-5 relative in
  t; at most 2 % may be (seed 5: 7 of 2000).  On every other ray the
  restatement's face is the reference's, t agrees to 8 x MEASURED_T_DEVIATION, and the point o + t d lies within 12 sqrt(3) u M of the
  face's plane, u = 2^-24, M the largest |corner - o| coordinate of the face: the accuracy csrc/meshray.hip sizes its margin from."""
  m = generic_soup()
  o, d = soup_rays()
  t, f, b, det = Q.cast(o, d, m['vertices'], m['faces'], details=True)
  t64, b64 = Q.moller_trumbore(o, d, m['vertices'], m['faces'])
  with np.errstate(all='ignore'):
    front = t64 > 0
    inside = front & (b64 > 1e-4).all(-1)                                             # the clear hits
    ts = np.sort(np.where(inside, t64, np.inf), 1)
    close = np.isfinite(ts[:, 1]) & (ts[:, 1] - ts[:, 0] <= 1e-5 * ts[:, 1])
    # a CANDIDATE is a face that could be the answer: on an edge or a corner to 1e-4 and not behind the nearest clear hit
    near_edge = front & (np.abs(b64) <= 1e-4).any(-1) & (b64 >= -1e-4).all(-1) & (t64 <= ts[:, :1] * (1 + 1e-5))
  ambiguous = near_edge.any(1) | close
  want = np.where(inside.any(1), np.where(inside, t64, np.inf).argmin(1), -1)
  keep = ~ambiguous
  print(f'{int(ambiguous.sum())} of {len(o)} rays ambiguous, {int((want[keep] >= 0).sum())} hits, {int((want[keep] < 0).sum())} misses')
  assert ambiguous.mean() <= 0.02 and (want[keep] >= 0).sum() > 1000 and (want[keep] < 0).sum() > 20
  assert np.array_equal(f[keep], want[keep])
  hit = keep & (want >= 0)
  rows = np.nonzero(hit)[0]
  ref = t64[rows, want[rows]]
  dev = np.abs(t[rows].astype(np.float64) - ref) / ref
  # the hit point against the face's plane
  v = m['vertices'].astype(np.float64)[m['faces'][want[rows]]]
  nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
  nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
  p = o[rows].astype(np.float64) + t[rows].astype(np.float64)[:, None] * d[rows].astype(np.float64)
  M = np.abs(v - o[rows].astype(np.float64)[:, None]).max((1, 2))
  off = np.abs(((p - v[:, 0]) * nrm).sum(-1)) / (12 * np.sqrt(3) * U24 * M)
  print(f'max |t - t64| / t64 = {dev.max():.3e} (8 x recorded: {8 * MEASURED_T_DEVIATION:.3e}), largest plane offset / bound {off.max():.3f}')
  assert dev.max() <= 8 * MEASURED_T_DEVIATION
  assert off.max() <= 1.
  assert (np.abs(b[rows].astype(np.float64) - b64[rows, want[rows]]).max(-1) <= 1e-4).all()
  assert np.array_equal(t[keep & (want < 0)], np.full((keep & (want < 0)).sum(), INF))


# ---- the rasteriser's restatement

@functools.lru_cache(maxsize=None)
def latlong_outside():
  """(mesh, raster restatement, raycast restatement with details, rays) of latlong_sphere(12) from VIEWS['outside'] at 47 x 61."""
  m = R.latlong_sphere(12, radius=0.6)
  eye, target, focal, near = VIEWS['outside']
  P, _ = projection('outside')
  ras = R.render(m, P, H, W, near)
  o, d = Q.pinhole_rays(R.pixtocam(focal, W, H), R.look_at(eye, target), H, W)
  ray = Q.cast(o.reshape(-1, 3), d.reshape(-1, 3), m['vertices'], m['faces'], t_min=near, details=True)
  return m, ras, ray, (o.reshape(-1, 3), d.reshape(-1, 3))


def test_the_two_restatements_agree_on_a_view():
  """raster_ref and raycast_ref on latlong_sphere(12), view `outside`, 47 x 61: the faces differ at no more than 1 % of the pixels
  (silhouette and edge ties only: the two tests round differently), and where they agree both depths are the float64 intersection of
  the pixel's ray with the face's plane: the ray caster's t to the plane offset its margin argument allows (12 sqrt(3) u M, divided by
  the cosine between ray and normal); the rasteriser's zc is printed next to it."""
  m, ras, (t, f, b, det), (o, d) = latlong_outside()
  rf = ras['face'].reshape(-1)
  differ = rf != f
  print(f'{int(differ.sum())} of {H * W} pixels differ, {int((f >= 0).sum())} hit')
  assert differ.mean() <= 0.01 and (f >= 0).sum() > 200 and (f < 0).sum() > 200
  agree = np.nonzero(~differ & (f >= 0))[0]
  v = m['vertices'].astype(np.float64)[m['faces'][f[agree]]]
  o64, d64 = o[agree].astype(np.float64), d[agree].astype(np.float64)
  nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
  nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
  t64 = ((v[:, 0] - o64) * nrm).sum(-1) / (d64 * nrm).sum(-1)
  M = np.abs(v - o64[:, None]).max((1, 2))
  bound = 12 * np.sqrt(3) * U24 * M / np.abs((d64 * nrm).sum(-1))
  err = np.abs(t[agree].astype(np.float64) - t64)
  print(f'ray caster: max |t - t64| {err.max():.3e}, largest error / bound {(err / bound).max():.3f}')
  assert (err <= bound).all()
  assert (np.abs(det['t64'][agree] - t[agree]) <= U24 * t[agree]).all()            # t is the float64 quotient rounded once
  zc = ras['depth'].reshape(-1)[agree].astype(np.float64)
  print(f'rasteriser (for the record; its own tests hold it): max |zc - t64| / t64 {(np.abs(zc - t64) / t64).max():.3e}')
  assert (np.abs(b[agree].astype(np.float64) - ras['bary'].reshape(-1, 3)[agree]) <= 1e-3).all()
