"""NumPy restatement of csrc/meshdist.hip (include/mnerf.h, "Mesh geometry"): the point-to-face squared distance, brute force, every
query against every face, in float32 in the contract's order of operations and the same again in float64; the sampler and its
integer mix; plain float64 point, segment and sampled-triangle distances to hold the formula against."""

import numpy as np

F32, F64 = np.float32, np.float64


def dot(x, y):
  return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(u, v):
  return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                   u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def seg_d2(p, u, v):
  """Squared distance of points p [N,3] to the segment (u, v) [3], in the dtype of p."""
  dt = p.dtype.type
  uv, up = v - u, p - u
  L = dot(uv, uv)
  t = np.zeros(p.shape[:-1], dtype=p.dtype)
  if L > 0:
    t = np.minimum(np.maximum(dot(up, uv) / L, dt(0)), dt(1))
  e = up - t[..., None] * uv
  return dot(e, e)


def face_d2(p, a, b, c):
  """Squared distance of points p [N,3] to the face (a, b, c), the contract's formula in the dtype of p (float32 or float64)."""
  with np.errstate(all='ignore'):
    d2 = np.fmin(np.fmin(seg_d2(p, a, b), seg_d2(p, b, c)), seg_d2(p, c, a))
    ab, ac = b - a, c - a
    n = cross(ab, ac)
    nn = dot(n, n)
    if nn > 0:
      ap, bp, cp, bc, ca = p - a, p - b, p - c, c - b, a - c
      s0, s1, s2 = dot(n, cross(ab, ap)), dot(n, cross(bc, bp)), dot(n, cross(ca, cp))
      h = dot(n, ap)
      plane = (h * h) / nn
      d2 = np.where((s0 >= 0) & (s1 >= 0) & (s2 >= 0), np.fmin(d2, plane), d2)
  return d2


def valid_faces(verts, faces):
  V = len(verts)
  ok = ((faces >= 0) & (faces < V)).all(1)
  ok[ok] = np.isfinite(verts[faces[ok]]).all((1, 2))
  return ok


NONE_KEY = np.uint64(0x7f800000ffffffff)


def point_mesh_distance(points, verts, faces, max_dist=None, dtype=F32):
  """(d2 [N] dtype, face [N] int32) by brute force: the minimum of (d2, face) in that order over the eligible faces.  In float32 this
  is the kernels' result bit for bit; dtype=float64 evaluates the same formula on the same float32 inputs, widened."""
  p = np.ascontiguousarray(points, dtype=F32).astype(dtype)
  v = np.ascontiguousarray(verts, dtype=F32).astype(dtype)
  N = len(p)
  best = np.full((N,), np.inf, dtype=dtype)
  face = np.full((N,), -1, dtype=np.int32)
  lim = dtype(np.inf) if max_dist is None else dtype(F32(max_dist) * F32(max_dist)) if dtype is F32 else F64(max_dist) * F64(max_dist)
  live = np.isfinite(p).all(1)
  ok = valid_faces(np.asarray(verts, dtype=F32), faces)
  for f in np.nonzero(ok)[0]:
    a, b, c = v[faces[f, 0]], v[faces[f, 1]], v[faces[f, 2]]
    with np.errstate(all='ignore'):
      d2 = face_d2(p, a, b, c)
      take = live & (d2 <= lim) & ((d2 < best) | ((face < 0) & (d2 <= best)))     # ascending f: the lowest id of equal d2 stays
    best[take], face[take] = d2[take], f
  return best, face


# ---- the sampler

def mix(x):
  x = np.asarray(x, dtype=np.uint32).copy()
  with np.errstate(over='ignore'):
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
  return x


def face_areas(verts, faces):
  """[T] float64: 0.5 |(b - a) x (c - a)| from the float32 corners widened, 0 for a face that is not valid."""
  v = np.asarray(verts, dtype=F32).astype(F64)
  ok = valid_faces(np.asarray(verts, dtype=F32), faces)
  out = np.zeros((len(faces),), dtype=F64)
  a, b, c = (v[faces[ok, k]] for k in range(3))
  n = cross(b - a, c - a)
  out[ok] = 0.5 * np.sqrt(dot(n, n))
  return out


def barycentrics(n, seed):
  """b [n,3] float32 of samples 0 .. n - 1."""
  i = np.arange(n, dtype=np.uint32)
  with np.errstate(over='ignore'):
    s = mix(np.uint32(seed))
    h1, h2 = mix(s + np.uint32(2) * i), mix(s + (np.uint32(2) * i + np.uint32(1)))
  r1 = (h1 >> np.uint32(8)).astype(F32) * F32(2. ** -24)
  r2 = (h2 >> np.uint32(8)).astype(F32) * F32(2. ** -24)
  fold = r1 > F32(1) - r2
  r1, r2 = np.where(fold, F32(1) - r1, r1), np.where(fold, F32(1) - r2, r2)
  return np.stack([(F32(1) - r1) - r2, r1, r2], -1).astype(F32)


def sample(verts, faces, cum, n, seed):
  """(points [n,3] float32, face [n] int32, b [n,3] float32) given the inclusive running sum `cum` [T] float64."""
  verts = np.asarray(verts, dtype=F32)
  u = ((np.arange(n, dtype=F64) + 0.5) / F64(n)) * cum[-1]
  k = np.minimum(np.searchsorted(cum, u, side='right'), len(cum) - 1)            # the first k with cum[k] > u
  b = barycentrics(n, seed)
  A, B, C = (verts[faces[k, j]] for j in range(3))
  pts = (b[:, 0:1] * A + b[:, 1:2] * B) + b[:, 2:3] * C
  return pts.astype(F32), k.astype(np.int32), b


# ---- plain float64 truths

def point_segment(p, u, v):
  """Distance of p [N,3] to the segment (u, v), float64, the textbook way."""
  p, u, v = (np.asarray(x, dtype=F64) for x in (p, u, v))
  d = v - u
  L = d @ d
  t = np.clip(((p - u) @ d) / L, 0., 1.) if L > 0 else np.zeros(len(p))
  return np.linalg.norm(p - (u + t[:, None] * d), axis=-1)


def sampled_triangle(p, a, b, c, steps):
  """min over a barycentric lattice of `steps` intervals a side of |p - x|, float64 [N]: an upper bound of the distance, within the
  lattice's step (the longest edge over `steps`) of it."""
  p, a, b, c = (np.asarray(x, dtype=F64) for x in (p, a, b, c))
  i, j = np.meshgrid(np.arange(steps + 1), np.arange(steps + 1), indexing='ij')
  keep = i + j <= steps
  u, v = i[keep] / steps, j[keep] / steps
  x = a + u[:, None] * (b - a) + v[:, None] * (c - a)
  return np.sqrt(((p[:, None, :] - x[None]) ** 2).sum(-1).min(1))


# ---- the inputs of the GPU tests (built once here so that the CPU test measures float32 against float64 on exactly them)

def soup(seed=11, flat=False):
  """(verts, faces): 300 random triangles in [-0.6, 0.6]^3; faces 50 .. 59 repeat 40 .. 49 (the lowest id must win); face 60 has three
  equal corners, 61 two equal, 62 exactly collinear ones; 70 .. 119 are slivers whose third corner is 1e-3 .. 1e-7 off the opposite
  edge; 120 has index -1, 121 index V, 122 a NaN corner, 123 an infinite one; 124 spans the whole box.  flat=True: z = 0."""
  rng = np.random.default_rng(seed)
  T = 300
  verts = rng.uniform(-0.6, 0.6, (3 * T + 2, 3)).astype(F32)
  faces = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
  faces[50:60] = faces[40:50]
  verts[faces[60, 1]] = verts[faces[60, 2]] = verts[faces[60, 0]]
  verts[faces[61, 1]] = verts[faces[61, 0]]
  verts[faces[62, 0]], verts[faces[62, 1]], verts[faces[62, 2]] = F32([-.25, .125, .5]), F32([0., .25, .25]), F32([.5, .5, -.25])
  for k, f in enumerate(range(70, 120)):
    a, b = verts[faces[f, 0]].astype(F64), verts[faces[f, 1]].astype(F64)
    d = np.cross(b - a, rng.normal(size=3))
    verts[faces[f, 2]] = (a + rng.uniform(0.1, 0.9) * (b - a) + 10. ** (-3 - 4 * k / 49.) * d / np.linalg.norm(d)).astype(F32)
  faces[120, 1], faces[121, 2] = -1, len(verts)
  verts[3 * T], verts[3 * T + 1] = F32([np.nan, 0., 0.]), F32([0.1, np.inf, 0.2])
  faces[122, 0], faces[123, 1] = 3 * T, 3 * T + 1
  verts[faces[124, 0]], verts[faces[124, 1]], verts[faces[124, 2]] = F32([-.6, -.6, -.6]), F32([.6, .6, -.6]), F32([.6, -.6, .6])
  if flat:
    verts[np.isfinite(verts[:, 2]), 2] = 0
  return verts, faces


def soup_box(verts, faces):
  c = verts[faces[valid_faces(verts, faces)]].reshape(-1, 3)
  return c.min(0), c.max(0)


def queries(verts, faces, cell, seed=12):
  """1500 queries [N,3] float32 for a soup: uniform in [-1, 1]^3 (some outside the grid), 200 on face centroids, 200 within 1e-4 of
  edge midpoints, 8 at exact cell corners of the grid of side `cell` at the soup's box, 6 at distance 50, one NaN, one infinite."""
  rng = np.random.default_rng(seed)
  ok = np.nonzero(valid_faces(verts, faces))[0]
  v64 = verts.astype(F64)
  f = rng.choice(ok, 200)
  cent = v64[faces[f]].mean(1)
  f = rng.choice(ok, 200)
  mid = 0.5 * (v64[faces[f, 0]] + v64[faces[f, 1]]) + rng.uniform(-1e-4, 1e-4, (200, 3)) / np.sqrt(3.)
  lo, _ = soup_box(verts, faces)
  corners = (lo[None] + F32(cell) * rng.integers(0, 5, (8, 3)).astype(F32)).astype(F32)
  far = rng.normal(size=(6, 3))
  far = 50. * far / np.linalg.norm(far, axis=-1, keepdims=True)
  odd = np.array([[np.nan, 0., 0.], [0., np.inf, 0.]])
  uni = rng.uniform(-1., 1., (1500 - 200 - 200 - 8 - 6 - 2, 3))
  q = np.concatenate([uni, cent, mid, corners, far, odd], 0).astype(F32)
  assert q.shape == (1500, 3)
  return q


def sparse_case(seed=13):
  """(verts, faces, queries, cell): two clusters of 20 faces each whose centres are 100 cells apart along x, 100 queries between them:
  many empty shells are walked."""
  rng = np.random.default_rng(seed)
  cell = 0.05
  tri = rng.uniform(-0.04, 0.04, (40, 3, 3))
  tri[20:, :, 0] += 100 * cell
  verts = tri.reshape(-1, 3).astype(F32)
  faces = np.arange(120, dtype=np.int32).reshape(40, 3)
  q = np.stack([rng.uniform(0., 100 * cell, 100), rng.uniform(-0.1, 0.1, 100), rng.uniform(-0.1, 0.1, 100)], -1).astype(F32)
  return verts, faces, q, cell
