"""Known answers of tests/raster_ref.py, the NumPy restatement that tests/test_gpu_raster.py holds csrc/raster.hip to: watertight
cover counts, pixel-aligned edges, the documented vertex caveat, and barycentrics / depth against a float64 ray-triangle
intersection.  No GPU."""

import numpy as np

from multinerf_amd import mesh
from tests import raster_ref as R

NEAR = 1e-3


def cover_counts(m, P, H, W):
  assert R.vertex_clearance(m['vertices'], P) >= 1e-3       # the precondition of every watertightness claim (include/mnerf.h, LIMIT)
  return R.visibility(m['vertices'], m['faces'], P, H, W, NEAR, counts=True)[1]


def test_inside_view_covers_every_pixel_exactly_once():
  """A closed sphere (528 faces) at 64 x 64 from a camera inside it: many faces lie behind or across the camera plane, nothing is
  clipped, and every pixel is covered by exactly one face."""
  m = R.latlong_sphere(12)
  assert m['faces'].shape == (528, 3)
  P = mesh.world_to_pixel(R.pixtocam(20., 64, 64), R.look_at((0.2, -0.1, 0.3), (1., 0.3, 0.2)))
  h = R.homogeneous(m['vertices'], P)[m['faces']]
  behind = (h[..., 2] <= 0).any(-1)
  assert behind.sum() > 100 and ((h[..., 2] <= 0).any(-1) & (h[..., 2] > 0).any(-1)).sum() > 10      # behind, and across
  assert (cover_counts(m, P, 64, 64) == 1).all()


def test_outside_views_cover_a_pixel_twice_or_not_at_all():
  m = R.latlong_sphere(12)
  rng = np.random.default_rng(3)
  for _ in range(6):
    eye = rng.normal(size=3)
    eye *= rng.uniform(2.5, 5.) / np.linalg.norm(eye)
    P = mesh.world_to_pixel(R.pixtocam(60., 64, 64), R.look_at(eye, rng.uniform(-0.3, 0.3, 3)))
    counts = cover_counts(m, P, 64, 64)
    assert set(np.unique(counts).tolist()) == {0, 2}        # front and back, never a crack (1) and never a double hit (3)


def aligned_quads():
  """Two quads of two triangles each that share an edge, at zc = 2, whose edges and diagonals pass exactly through pixel centres
  under P = [I | 0]: 17 x 17 centres each."""
  z = 2.
  corners = [(2.5, 2.5), (19.5, 2.5), (36.5, 2.5), (2.5, 19.5), (19.5, 19.5), (36.5, 19.5)]
  verts = np.array([(x * z, y * z, z) for x, y in corners], np.float32)
  faces = np.array([(0, 1, 4), (0, 4, 3), (1, 2, 5), (1, 5, 4)], np.int32)
  return dict(vertices=verts, normals=np.zeros_like(verts), faces=faces), np.eye(3, 4, dtype=np.float32)


def test_pixel_aligned_quads_cover_578_pixels_once_each():
  m, P = aligned_quads()
  for faces in (m['faces'], m['faces'][:, ::-1]):           # either orientation
    vis, counts = R.visibility(m['vertices'], faces, P, 24, 40, NEAR, counts=True)
    assert (counts <= 1).all() and counts.sum() == 578
    ys, xs = np.nonzero(counts)
    assert xs.max() - xs.min() == 33 and ys.max() - ys.min() == 16
    depth = (vis[counts == 1] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert (depth == 2.).all()


def test_the_vertex_caveat_is_a_recorded_case():
  """include/mnerf.h, LIMIT: the south pole of the sphere projected within rounding of the pixel centre (27.5, 33.5).  The fan's 24
  rounded edge lines do not meet in one point and that ONE pixel is miscounted (here 5 faces claim it; other cameras give 0, 4 or
  7); every other pixel is covered exactly once.  Recorded, not a failure: the cure, fixed-point vertices, is out of scope."""
  m = R.latlong_sphere(12)
  K = np.array([[20., 0., 27.5], [0., 20., 33.5], [0., 0., 1.]])
  c2w = R.look_at((0.10956934985716349, -0.18417062898890377, -0.36722118085104427), (0., 0., -1.), up=(0., 1., 0.))
  P = mesh.world_to_pixel(np.linalg.inv(K), c2w)
  pole = R.projected_vertices(m['vertices'], P)[-1]
  assert np.abs(pole - (27.5, 33.5)).max() < 1e-5 and R.vertex_clearance(m['vertices'], P) < 1e-3
  counts = R.visibility(m['vertices'], m['faces'], P, 64, 64, NEAR, counts=True)[1]
  assert np.argwhere(counts != 1).tolist() == [[33, 27]]
  assert counts[33, 27] == 5


def test_barycentrics_and_depth_against_a_float64_ray_intersection():
  """bary = E_i / S and depth = |det| / S against the intersection of the pixel's ray with its face's plane in float64.  The ray is
  camera_utils.pixels_to_rays': origin o, direction R diag(1, -1, -1) pixtocam (x + .5, y + .5, 1), not normalised, so the ray
  parameter IS zc.  Bound: h, the cross products and E each carry a few float32 roundings of numbers of the size of the products
  that are subtracted; on this scene the subtracted products are below 2^12 times the result, which gives 2^12 * 2^-23 * (a few) <
  5e-3 as the relative bound on zc and the absolute one on the barycentrics; measured: 7e-5 and 7e-5."""
  m = R.latlong_sphere(12)
  H, W, focal = 47, 61, 55.
  ptc, c2w = R.pixtocam(focal, W, H), R.look_at((2.5, 1.5, 1.0), (0.1, 0., -0.1))
  P = mesh.world_to_pixel(ptc, c2w)
  out = R.render(m, P, H, W, NEAR)
  ys, xs = np.nonzero(out['face'] >= 0)
  assert len(ys) > 300
  d = (c2w[:, :3] @ np.diag([1., -1., -1.]) @ ptc @ np.stack([xs + .5, ys + .5, np.ones(len(xs))])).T
  o = c2w[:, 3]
  v = m['vertices'].astype(np.float64)[m['faces'][out['face'][ys, xs]]]
  normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
  t = ((v[:, 0] - o) * normal).sum(-1) / (d * normal).sum(-1)
  p = o + t[:, None] * d
  area = lambda a, b, c: (np.cross(b - a, c - a) * normal).sum(-1)
  bary = np.stack([area(p, v[:, 1], v[:, 2]), area(v[:, 0], p, v[:, 2]), area(v[:, 0], v[:, 1], p)], -1) / area(v[:, 0], v[:, 1], v[:, 2])[:, None]
  ez, eb = np.abs(out['depth'][ys, xs] / t - 1).max(), np.abs(out['bary'][ys, xs] - bary).max()
  print(f'{len(ys)} pixels: depth relative {ez:.3e}, barycentrics absolute {eb:.3e}')
  assert ez < 5e-3 and eb < 5e-3
  assert (bary > -5e-3).all() and np.abs(out['bary'][ys, xs].sum(-1) - 1).max() < 1e-6
  assert (out['acc'] == (out['face'] >= 0)).all() and (out['depth'][out['face'] < 0] == 0).all()
  # the shaded normal: the blend of unit vertex normals of a sphere is the direction of the point, to the faces' size
  n = out['normals'][ys, xs]
  assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-6 and np.abs(n - p / np.linalg.norm(p, axis=-1, keepdims=True)).max() < 0.05
  assert np.array_equal(out['rgb'][ys, xs], np.float32(0.5) + np.float32(0.5) * n) and (out['rgb'][out['face'] < 0] == 1).all()
