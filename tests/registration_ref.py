"""NumPy restatement of csrc/meshreg.hip (include/mnerf.h, "Mesh registration"): the closest point on a face and the face's unit
normal in the contract's order of operations (float32, and the same again in float64), the 47 terms of the ICP sums, the polygonal
crop, and a plain float64 ICP with brute-force closest points that the registration is held against; the test shape."""

import numpy as np

from tests import geometry_ref as G

F32, F64 = np.float32, np.float64
ICP_SUMS = 47


def _seg(p, u, v):
  """(dot(e, e), t) of seg(p, u, v), rows of [...,3] arrays, in their dtype."""
  dt = p.dtype.type
  uv, up = v - u, p - u
  L = G.dot(uv, uv)
  with np.errstate(all='ignore'):
    t = np.where(L > 0, np.minimum(np.maximum(G.dot(up, uv) / L, dt(0)), dt(1)), dt(0)).astype(p.dtype)
  e = up - t[..., None] * uv
  return G.dot(e, e), t


def unit(n, nn):
  """n / sqrt(nn) where nn is positive and finite, else 0."""
  ok = (nn > 0) & np.isfinite(nn)
  with np.errstate(all='ignore'):
    out = n / np.sqrt(nn)[..., None]
  return np.where(ok[..., None], out, n.dtype.type(0)).astype(n.dtype)


def closest_on_faces(p, a, b, c):
  """(x, nrm) [...,3] for points p and the corners a, b, c [...,3] of their (valid) faces, in the dtype of p."""
  with np.errstate(all='ignore'):
    (s0, t0), (s1, t1), (s2, t2) = _seg(p, a, b), _seg(p, b, c), _seg(p, c, a)
    best, k = s0.copy(), np.zeros(p.shape[:-1], dtype=np.int64)
    take = s1 < best
    best, k = np.where(take, s1, best), np.where(take, 1, k)
    take = s2 < best
    best, k = np.where(take, s2, best), np.where(take, 2, k)
    k3 = k[..., None]
    u, v = np.where(k3 == 0, a, np.where(k3 == 1, b, c)), np.where(k3 == 0, b, np.where(k3 == 1, c, a))
    t = np.where(k == 0, t0, np.where(k == 1, t1, t2))
    x = u + t[..., None] * (v - u)
    ab, ac = b - a, c - a
    n = G.cross(ab, ac)
    nn = G.dot(n, n)
    ap, bp, cp, bc, ca = p - a, p - b, p - c, c - b, a - c
    g0, g1, g2 = G.dot(n, G.cross(ab, ap)), G.dot(n, G.cross(bc, bp)), G.dot(n, G.cross(ca, cp))
    h = G.dot(n, ap)
    plane = (nn > 0) & (g0 >= 0) & (g1 >= 0) & (g2 >= 0) & ((h * h) / nn <= best)
    x = np.where(plane[..., None], p - (h / nn)[..., None] * n, x)
  return x.astype(p.dtype), unit(n, nn)


def closest(points, face, verts, faces, vnormals=None, dtype=F32):
  """(x, nrm) [N,3] of mnr_mesh_closest: in float32 the kernel's result bit for bit; dtype=float64 evaluates the same formula on the
  same float32 inputs, widened."""
  pts = np.ascontiguousarray(points, dtype=F32)
  p, v = pts.astype(dtype), np.ascontiguousarray(verts, dtype=F32).astype(dtype)
  face = np.asarray(face, dtype=np.int64)
  ok = (face >= 0) & (face < len(faces)) & np.isfinite(pts).all(1)
  ok[ok] = G.valid_faces(np.asarray(verts, dtype=F32), faces[face[ok]])
  x, nrm = p.copy(), np.zeros_like(p)
  f = faces[face[ok]]
  x[ok], nrm[ok] = closest_on_faces(p[ok], v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
  if vnormals is not None:
    point = ok.copy()
    point[ok] = (f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2])
    vn = np.ascontiguousarray(vnormals, dtype=F32).astype(dtype)[faces[face[point], 0]]
    with np.errstate(all='ignore'):
      length = np.sqrt(G.dot(vn, vn))
      fine = (length > 0) & np.isfinite(length)
      nrm[point] = np.where(fine[:, None], vn / length[:, None], dtype(0))
  return x, nrm


def face_normals(verts, faces):
  """[T,3] float32 of mnr_mesh_face_normals."""
  v = np.asarray(verts, dtype=F32)
  ok = G.valid_faces(v, faces)
  out = np.zeros((len(faces), 3), dtype=F32)
  a, b, c = (v[faces[ok, k]] for k in range(3))
  n = G.cross(b - a, c - a)
  out[ok] = unit(n, G.dot(n, n))
  return out


def icp_terms(p, x, nrm, keep, centre):
  """[n,47] float64: the terms of mnr_icp_sums, one row a correspondence (zero where keep is 0), in the header's layout and order of
  operations; their column sums are the sums."""
  p, x, n = (np.asarray(a, dtype=F32).astype(F64) for a in (p, x, nrm))
  c = np.asarray(centre, dtype=F64)
  pc, xc, d = p - c, x - c, p - x
  r = G.dot(d, n)
  J = np.concatenate([G.cross(pc, n), n], 1)
  cols = [np.ones(len(p))] + [pc[:, k] for k in range(3)] + [xc[:, k] for k in range(3)]
  cols += [pc[:, k] * xc[:, l] for k in range(3) for l in range(3)]
  cols += [G.dot(pc, pc), G.dot(xc, xc), G.dot(d, d), r * r]
  cols += [J[:, k] * J[:, l] for k in range(6) for l in range(k, 6)]
  cols += [J[:, k] * r for k in range(6)]
  terms = np.stack(cols, 1) if len(p) else np.zeros((0, ICP_SUMS))
  assert terms.shape[1] == ICP_SUMS
  return terms * (np.asarray(keep) != 0)[:, None]


UVW = {0: (1, 2, 0), 1: (0, 2, 1), 2: (0, 1, 2)}


def crop_polygon(points, polygon, axis, w_min, w_max):
  """bool [n] of mnr_crop_polygon: float64 throughout."""
  p = np.asarray(points, dtype=F32).astype(F64)
  poly = np.asarray(polygon, dtype=F64)
  iu, iv, iw = UVW[axis]
  pu, pv, pw = p[:, iu], p[:, iv], p[:, iw]
  odd = np.zeros(len(p), dtype=bool)
  m = len(poly)
  for i in range(m):
    (au, av), (bu, bv) = poly[i], poly[(i + 1) % m]
    with np.errstate(all='ignore'):
      hit = ((av > pv) != (bv > pv)) & (pu < ((bu - au) * (pv - av)) / (bv - av) + au)
    odd ^= hit
  return (w_min <= pw) & (pw <= w_max) & odd


# ---- a plain float64 ICP, brute force

def brute_closest(p, verts, faces, max_dist):
  """(x, nrm, inlier) in float64: every point against every face (the contract's formula evaluated in float64)."""
  p, v = np.asarray(p, dtype=F64), np.asarray(verts, dtype=F64)
  shape = (len(p), len(faces), 3)
  q = np.broadcast_to(p[:, None, :], shape)
  xf, nf = closest_on_faces(q, *(np.broadcast_to(v[faces[:, k]][None], shape) for k in range(3)))
  d2 = ((q - xf) ** 2).sum(-1)
  f = d2.argmin(1)                                                 # (the first of equal minima: the lowest face)
  rows = np.arange(len(p))
  x, nrm, best = xf[rows, f], nf[rows, f], d2[rows, f]
  return x, nrm, best <= max_dist ** 2


def rodrigues(w):
  th = np.linalg.norm(w)
  K = np.array([[0., -w[2], w[1]], [w[2], 0., -w[0]], [-w[1], w[0], 0.]])
  if th < 1e-12:
    return np.eye(3) + K
  return np.eye(3) + np.sin(th) / th * K + (1. - np.cos(th)) / th ** 2 * (K @ K)


def icp(src, verts, faces, max_dist, mode, iters, with_scale=False, init=None):
  """(T [4,4], history of (fitness, rmse)): `iters` updates of a textbook ICP in float64, and the evaluation after the last."""
  T = np.eye(4) if init is None else np.array(init, dtype=F64)
  src = np.asarray(src, dtype=F64)
  history = []
  for it in range(iters + 1):
    p = src @ T[:3, :3].T + T[:3, 3]
    x, n, keep = brute_closest(p, verts, faces, max_dist)
    history.append((keep.mean(), np.sqrt(((p - x)[keep] ** 2).sum(1).mean())))
    if it == iters:
      break
    p, x, n = p[keep], x[keep], n[keep]
    D = np.eye(4)
    if mode == 'point':
      mp, mx = p.mean(0), x.mean(0)
      U, sv, Vt = np.linalg.svd((p - mp).T @ (x - mx) / len(p))
      sign = np.array([1., 1., np.sign(np.linalg.det(Vt.T @ U.T))])
      R = Vt.T @ np.diag(sign) @ U.T
      s = (sv * sign).sum() / ((p - mp) ** 2).sum(1).mean() if with_scale else 1.
      D[:3, :3], D[:3, 3] = s * R, mx - s * R @ mp
    else:
      J = np.concatenate([np.cross(p, n), n], 1)                   # rotation about the origin
      r = ((p - x) * n).sum(1)
      xi = np.linalg.solve(J.T @ J, -J.T @ r)
      D[:3, :3], D[:3, 3] = rodrigues(xi[:3]), xi[3:]
    T = D @ T
  return T, history


# ---- the test shape and its fixed perturbation

def icosphere(subdivisions=2):
  """(verts [V,3] float64 on the unit sphere, faces [T,3] int32): 162 vertices and 320 faces at two subdivisions."""
  g = (1. + np.sqrt(5.)) / 2.
  v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
  f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
       (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
  v = [np.array(x, dtype=F64) / np.linalg.norm(x) for x in v]
  for _ in range(subdivisions):
    mid, out = {}, []

    def midpoint(i, j):
      key = (min(i, j), max(i, j))
      if key not in mid:
        m = v[i] + v[j]
        v.append(m / np.linalg.norm(m))
        mid[key] = len(v) - 1
      return mid[key]
    for a, b, c in f:
      ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
      out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    f = out
  return np.array(v), np.array(f, dtype=np.int32)


def shape():
  """(verts float32, faces int32): the icosphere subdivided twice, scaled by (1, 0.7, 0.5), with one Gaussian bump (height 0.15, width
  0.35, around the direction (0.6, 0.64, 0.48)) pushed out along the radius, so that no rotation maps the shape onto itself."""
  v, f = icosphere(2)
  bump = 1. + 0.15 * np.exp(-((v - np.array([0.6, 0.64, 0.48])) ** 2).sum(1) / (2 * 0.35 ** 2))
  return (v * bump[:, None] * np.array([1., 0.7, 0.5])).astype(F32), f


def perturbation():
  """P [4,4] float64: the rotation of 5 degrees about (0.3, -0.5, 0.8) and the translation (0.05, -0.03, 0.04)."""
  axis = np.array([0.3, -0.5, 0.8])
  P = np.eye(4)
  P[:3, :3] = rodrigues(np.deg2rad(5.) * axis / np.linalg.norm(axis))
  P[:3, 3] = [0.05, -0.03, 0.04]
  return P


def l_polygon():
  """A concave L-shaped hexagon [6,2] whose corners are exact in float32."""
  return np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.], [0., 0.], [0., 0.5], [-0.5, 0.5]], dtype=F64)
