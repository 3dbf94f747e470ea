"""NumPy restatement of the mesh ray caster's contract (include/mnerf.h "Mesh ray casting", csrc/meshray.hip): the watertight hit
test of every ray against every face, with no grid and no walk, and the lexicographic (t bits, face) minimum.  float32 in the
header's order (NumPy rounds every product and sum to float32 and never contracts), the three edge functions, det, t and the
barycentrics in float64 as the header says, so the kernel's buffers are held to these bit for bit."""

import numpy as np

F = np.float32
NONE = np.uint64(0x7f800000ffffffff)                         # (bits(+inf) << 32) | all ones


def shear(origins, directions):
  """dict(kx, ky, kz [n] int, Sx, Sy, Sz [n] float32, ok [n]) of every ray."""
  o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
  n = np.arange(len(d))
  a = np.abs(d)
  kz = np.zeros(len(d), np.int64)
  kz[a[:, 1] > a[:, 0]] = 1
  kz[a[:, 2] > np.maximum(a[:, 0], a[:, 1])] = 2               # the lowest index among equal magnitudes
  kx, ky = (kz + 1) % 3, (kz + 2) % 3
  dz = d[n, kz]
  swap = dz < 0
  kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
  with np.errstate(all='ignore'):
    Sx, Sy, Sz = d[n, kx] / dz, d[n, ky] / dz, F(1) / dz
  ok = np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & (dz != 0) & np.isfinite(Sz)
  return dict(kx=kx, ky=ky, kz=kz, Sx=Sx, Sy=Sy, Sz=Sz, ok=ok)


def valid_faces(verts, faces):
  """[T] bool: the three indices inside the vertices and the nine coordinates finite."""
  verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
  inside = ((faces >= 0) & (faces < len(verts))).all(-1)
  if len(verts) == 0:
    return inside & False
  return inside & np.isfinite(verts[np.where(inside[:, None], faces, 0)]).all((1, 2))


def hits(origins, directions, verts, faces, t_min=0., t_max=np.inf, cull='none'):
  """dict(t [n,T] float32, eligible [n,T], U, V, W, det [n,T] float64, t64 [n,T] float64 the quotient before its rounding) of every ray
  against every face: the hit test itself.  Meant for a chunk of faces that fits in memory."""
  o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
  verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
  sh = shear(o, d)
  valid = valid_faces(verts, faces)
  n = np.arange(len(o))
  corners = verts[np.where(valid[:, None], faces, 0)] if len(verts) else np.zeros((len(faces), 3, 3), F)      # [T,3 corners,3]
  with np.errstate(all='ignore'):
    P = corners[None] - o[:, None, None, :]                                                                 # [n,T,3,3]: a - o
    pick = lambda k: np.take_along_axis(P, np.broadcast_to(k[:, None, None, None], P.shape[:3] + (1,)), -1)[..., 0]     # [n,T,3]
    Pk = pick(sh['kz'])
    X = pick(sh['kx']) - sh['Sx'][:, None, None] * Pk
    Y = pick(sh['ky']) - sh['Sy'][:, None, None] * Pk
    Z = sh['Sz'][:, None, None] * Pk
    X, Y, Z = X.astype(np.float64), Y.astype(np.float64), Z.astype(np.float64)
    (Ax, Bx, Cx), (Ay, By, Cy), (Az, Bz, Cz) = (np.moveaxis(v, -1, 0) for v in (X, Y, Z))
    U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
    neg, pos = (U < 0) | (V < 0) | (W < 0), (U > 0) | (V > 0) | (W > 0)
    det = (U + V) + W
    inside = ~(neg & pos) & (det != 0)
    if cull == 'back':
      inside &= det > 0
    t64 = ((U * Az + V * Bz) + W * Cz) / det
    t = t64.astype(F)
  c64 = corners.astype(np.float64)
  with np.errstate(all='ignore'):
    area = (np.cross(c64[:, 1] - c64[:, 0], c64[:, 2] - c64[:, 0]) != 0).any(-1)                              # the face has area
  eligible = inside & (t > F(t_min)) & (t <= F(t_max)) & np.isfinite(t) & (valid & area)[None] & sh['ok'][:, None]
  return dict(t=t, eligible=eligible, U=U, V=V, W=W, det=det, t64=t64)


def cast(origins, directions, verts, faces, t_min=0., t_max=np.inf, cull='none', chunk=None, details=False):
  """(t [n] float32, face [n] int32, bary [n,3] float32) of mnr_mesh_raycast: the minimum of (bits(t) << 32) | face over the eligible
  faces; +inf, -1 and 0 where there is none.  details=True appends dict(t64 [n] float64: the winner's quotient before its rounding,
  count [n]: the number of eligible faces)."""
  o = np.asarray(origins, F).reshape(-1, 3)
  faces = np.asarray(faces, np.int64).reshape(-1, 3)
  n, T = len(o), len(faces)
  chunk = chunk or max(1, (1 << 20) // max(n, 1))
  best = np.full(n, NONE, np.uint64)
  bary = np.zeros((n, 3), F)
  t64 = np.full(n, np.inf)
  count = np.zeros(n, np.int64)
  rows = np.arange(n)
  for start in range(0, T, chunk):
    ids = np.arange(start, min(start + chunk, T))
    h = hits(o, directions, verts, faces[ids], t_min, t_max, cull)
    key = (np.ascontiguousarray(h['t']).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)[None]
    key = np.where(h['eligible'], key, NONE)
    k = key.argmin(1)
    kmin = key[rows, k]
    better = kmin < best
    with np.errstate(all='ignore'):
      l = np.stack([(h[c][rows, k] / h['det'][rows, k]).astype(F) for c in 'UVW'], -1)
    bary[better], t64[better] = l[better], h['t64'][rows, k][better]
    best = np.minimum(best, kmin)
    count += h['eligible'].sum(1)
  t = np.ascontiguousarray((best >> np.uint64(32)).astype(np.uint32)).view(F)
  face = (best & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
  out = (t, face, bary)
  return out + (dict(t64=t64, count=count),) if details else out


def pinhole_rays(pixtocam, camtoworld, H, W):
  """(origins, directions) [H,W,3] float32 of the pixel centres of a perspective camera: directions = R diag(1, -1, -1) pixtocam
  (x + .5, y + .5, 1) (camera_utils.pixels_to_rays' formula, evaluated in float64 and rounded once; they are NOT normalised, the
  camera-space z of every direction is -1), origins the eye."""
  K, c2w = np.asarray(pixtocam, np.float64).reshape(3, 3), np.asarray(camtoworld, np.float64)[:3, :4]
  ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
  cam = np.stack([xs, ys, np.ones_like(xs)], -1) @ K.T * np.array([1., -1., -1.])
  d = cam @ c2w[:, :3].T
  return np.broadcast_to(c2w[:, 3], d.shape).astype(F), d.astype(F)


def moller_trumbore(origins, directions, verts, faces):
  """(t [n,T], b [n,T,3]) float64: the textbook Moller-Trumbore intersection of every ray with every face's plane, NaN where the ray
  is parallel to it; b are the barycentrics of the point (any sign).  An independent formula, for the brute-force comparison."""
  o, d = np.asarray(origins, np.float64).reshape(-1, 1, 3), np.asarray(directions, np.float64).reshape(-1, 1, 3)
  v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
  a, e1, e2 = v[None, :, 0], (v[:, 1] - v[:, 0])[None], (v[:, 2] - v[:, 0])[None]
  with np.errstate(all='ignore'):
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    det = np.where(det == 0, np.nan, det)
    s = o - a
    u = (s * p).sum(-1) / det
    q = np.cross(s, e1)
    w = (d * q).sum(-1) / det
    t = (e2 * q).sum(-1) / det
  return t, np.stack([1. - u - w, u, w], -1)
