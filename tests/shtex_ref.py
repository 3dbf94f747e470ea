"""NumPy restatement of include/mnerf.h's "View-dependent texture" section (csrc/shtex.hip): the basis in both precisions, the weight,
the fit (float64, the same order of operations, the same fallbacks) and the shading pass (float32, the same order).  The blend,
the normalisation and float32 itself are imported from tests/raster_ref.py.  Its bilinear lookup cannot be: there it is not a function
but ten lines inside `shade`, which needs a visibility buffer and a projection, and that file stays as it is.  So `shade` below
repeats those lines, one to one, on 3 K planes instead of 3; tests/test_shtex_cpu.py holds the two together (at degree 0 with
coefficients colour / C0 the two restatements must give the same image to rounding)."""

import numpy as np

from tests.raster_ref import F, _blend, _normalise

D64 = np.float64
C0, C1, C2A, C2B, C2C = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396


def _basis(d, degree, T):
  x, y, z = d[..., 0], d[..., 1], d[..., 2]
  cols = [np.full(x.shape, T(C0))]
  if degree >= 1:
    cols += [T(C1) * y, T(C1) * z, T(C1) * x]
  if degree >= 2:
    cols += [T(C2A) * (x * y), T(C2A) * (y * z), T(C2B) * (T(3) * (z * z) - T(1)), T(C2A) * (x * z), T(C2C) * (x * x - y * y)]
  return np.stack(cols, -1)


def basis64(dirs, degree):
  """Y [D,K] float64 of float32 directions: the host table."""
  return _basis(np.asarray(dirs, F).astype(D64), degree, D64)


def basis32(d, degree):
  """Y [...,K] float32: the shading pass's evaluation."""
  return _basis(np.asarray(d, F), degree, F)


def closed_form(d, degree):
  """The same functions from their textbook definitions in float64, via polar angles: an independent check of the table."""
  d = np.asarray(d, D64)
  th, ph = np.arccos(np.clip(d[..., 2], -1, 1)), np.arctan2(d[..., 1], d[..., 0])
  s, c = np.sin(th), np.cos(th)
  cols = [np.full(th.shape, np.sqrt(1 / (4 * np.pi)))]
  if degree >= 1:
    k = np.sqrt(3 / (4 * np.pi))
    cols += [k * s * np.sin(ph), k * c, k * s * np.cos(ph)]
  if degree >= 2:
    k = np.sqrt(15 / (16 * np.pi))
    cols += [k * s * s * np.sin(2 * ph), 2 * k * s * c * np.sin(ph), np.sqrt(5 / (16 * np.pi)) * (3 * c * c - 1), 2 * k * s * c * np.cos(ph),
             k * s * s * np.cos(2 * ph)]
  return np.stack(cols, -1)


def weights(dirs, normals):
  """w [n,D] float32."""
  d, n = np.asarray(dirs, F)[None], np.asarray(normals, F)[:, None]
  with np.errstate(all='ignore'):
    a = -((d[..., 0] * n[..., 0] + d[..., 1] * n[..., 1]) + d[..., 2] * n[..., 2])
    return np.where(a > 0, np.where(a < 1, a, F(1)), F(0)).astype(F)


SOLVED, MEAN, EMPTY = 0, 1, 2


def fit(dirs, normals, rgb, degree, lam, return_status=False):
  """coef [n,K,3] float32 of rgb [n,D,3] float32: every texel scalar by scalar in the contract's order (the loops run over the
  contract's indices, each operation on all texels at once; a skipped direction adds +0, which changes no sum that started at +0).
  With return_status also what happened to each texel: SOLVED, MEAN (the weighted mean colour as a constant) or EMPTY (zeros)."""
  Y = basis64(dirs, degree)
  w = weights(dirs, normals)
  rgb = np.asarray(rgb, F)
  n, K = len(w), Y.shape[1]
  M, b, s, sw = np.zeros((K, K, n), D64), np.zeros((K, 3, n), D64), np.zeros((3, n), D64), np.zeros(n, D64)
  used = np.zeros(n, bool)
  with np.errstate(all='ignore'):
    for k in range(w.shape[1]):
      use = (w[:, k] > 0) & np.isfinite(rgb[:, k]).all(-1)
      used |= use
      wk, c = np.where(use, w[:, k], F(0)).astype(D64), np.where(use[:, None], rgb[:, k], F(0)).astype(D64).T
      for i in range(K):
        t = wk * Y[k, i]
        for j in range(i, K):
          M[i, j] += t * Y[k, j]
        b[i] += t * c
      sw = sw + wk
      s += wk * c
    tr = M[0, 0].copy()
    for i in range(1, K):
      tr = tr + M[i, i]
    mu = (D64(lam) * tr) / D64(K)
    for i in range(1, K):
      M[i, i] += mu
    ok = np.ones(n, bool)
    G = np.zeros((K, K, n), D64)
    for i in range(K):
      for j in range(i + 1):
        v = M[j, i].copy()
        for p in range(j):
          v = v - G[i, p] * G[j, p]
        if j < i:
          G[i, j] = v / G[j, j]
        else:
          ok &= (v > 0) & np.isfinite(v)
          G[i, i] = np.sqrt(v)
    out = np.zeros((n, K, 3), F)
    for ch in range(3):
      x = np.zeros((K, n), D64)
      for i in range(K):
        v = b[i, ch].copy()
        for p in range(i):
          v = v - G[i, p] * x[p]
        x[i] = v / G[i, i]
      for i in range(K - 1, -1, -1):
        v = x[i].copy()
        for p in range(i + 1, K):
          v = v - G[p, i] * x[p]
        x[i] = v / G[i, i]
      out[:, :, ch] = x.T.astype(F)
    ok &= np.isfinite(out).all((1, 2))
    mean = ((s / sw) / Y[0, 0]).T.astype(F)                   # [n,3]
    fallback = np.zeros((n, K, 3), F)
    fallback[:, 0] = np.where(np.isfinite(mean), mean, F(0))
    coef = np.where(ok[:, None, None], out, fallback)
    coef = np.where(used[:, None, None], coef, F(0))
  status = np.where(used, np.where(ok, SOLVED, MEAN), EMPTY)
  return (coef, status) if return_status else coef


def shade(verts, faces, face, bary, uv, sh, origin, rgb, F=F, return_points=False):
  """rgb [H,W,3] float32 with the pixels that show a face overwritten, as mnr_shtex_shade does it.  F=np.float64 runs the same
  formulas on the same float32 inputs in float64: the yardstick of the float32 shading error.  return_points adds (ys, xs, X, d),
  the shaded pixels with their surface points and view directions."""
  verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
  sh, out = np.asarray(sh, F), np.array(rgb, F)
  Ht, Wt, K = sh.shape[:3]
  degree = {1: 0, 4: 1, 9: 2}[K]
  f = np.asarray(face, np.int64)
  hit = (f >= 0) & (f < len(faces))
  if len(faces):
    ids_all = faces[np.where(hit, f, 0)]
    hit &= ((ids_all >= 0) & (ids_all < len(verts))).all(-1)
  ys, xs = np.nonzero(hit)
  if len(ys) == 0:
    return (out, (ys, xs, np.zeros((0, 3), F), np.zeros((0, 3), F))) if return_points else out
  fi, l = f[ys, xs], np.asarray(bary, F)[ys, xs]
  with np.errstate(all='ignore'):
    X = _blend(l, verts[faces[fi]])
    d, unit = _normalise(X - np.asarray(origin, F))
    d = np.where(unit[:, None], d, np.asarray([0, 0, 1], F))
    Y = _basis(d, degree, F)
    t = _blend(l, np.asarray(uv, F).reshape(-1, 3, 2)[fi])
    x, y = t[:, 0] * F(Wt) - F(0.5), (F(1) - t[:, 1]) * F(Ht) - F(0.5)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None, None], (y - yf)[:, None, None]
    xi = np.clip(np.nan_to_num(xf, nan=-1.), -1, Wt).astype(np.int64)
    yi = np.clip(np.nan_to_num(yf, nan=-1.), -1, Ht).astype(np.int64)
    xa, xb, ya, yb = np.clip(xi, 0, Wt - 1), np.clip(xi + 1, 0, Wt - 1), np.clip(yi, 0, Ht - 1), np.clip(yi + 1, 0, Ht - 1)
    top = (F(1) - fx) * sh[ya, xa] + fx * sh[ya, xb]
    bot = (F(1) - fx) * sh[yb, xa] + fx * sh[yb, xb]
    val = (F(1) - fy) * top + fy * bot                      # [n,K,3]
    r = Y[:, 0, None] * val[:, 0]
    for j in range(1, K):
      r = r + Y[:, j, None] * val[:, j]
    out[ys, xs] = np.where(r > 0, np.where(r < 1, r, F(1)), F(0))
  return (out, (ys, xs, X, d)) if return_points else out


# ---- the analytic colour field of the end-to-end tests: exactly degree 2 in the view direction, coefficients affine in position

def field_coefficients(points, degree=2, seed=3):
  """coef [n,K,3] float64 = A + B p: the constant term gives a colour around 0.5, the others |A| <= 0.18 and |B| <= 0.06 an entry.  For
  |p| <= 1 the view-dependent part swings by about +-0.3 around that and stays inside (0, 1): the tests that rely on it assert that
  nothing clips."""
  rng = np.random.default_rng(seed)
  K = (degree + 1) ** 2
  A, B = rng.uniform(-0.18, 0.18, (K, 3)), rng.uniform(-0.06, 0.06, (K, 3, 3))
  A[0], B[0] = rng.uniform(0.45, 0.55, 3) / C0, B[0] * 0.1 / C0
  return A[None] + np.einsum('kcd,nd->nkc', B, np.asarray(points, D64))


def field_colour(points, dirs, degree=2, seed=3):
  """rgb [n,3] float64 of the field at points [n,3] seen along the unit directions dirs [n,3]."""
  Y = _basis(np.asarray(dirs, D64), degree, D64)
  return np.einsum('nk,nkc->nc', Y, field_coefficients(points, degree, seed))


# The largest deviation tests/test_shtex_cpu.py finds (and asserts): of the restatement's coefficients from the field's on 42
# directions at lam = 0 (float32 colours in, one float32 rounding out), and of the float32 shading pass from its float64 evaluation on
# the same inputs.  tests/test_gpu_shtex.py builds its end-to-end bound from them: a coefficient error e_j changes a colour by at most
# e_j max|Y_j|, summed over the basis (SUM_MAX_BASIS).
FIT_DEVIATION = 5.0e-7           # measured 4.859e-07 (2000 texels, random unit normals and the six axes)
SHADE_F32_ERROR = 2.5e-7         # measured 2.204e-07 (80-face icosphere, cell 5, three cameras of 48 x 40)
SUM_MAX_BASIS = C0 + 3 * C1 + 3 * C2A / 2 + 2 * C2B + C2C


def bake(m, c, dirs, degree, lam, colour, filter=0.):
  """(sh [H,W,K,3] float32, uv [T,3,2], layout) of a host mesh: the SH part of mesh.bake_texture restated with tests/atlas_ref.py
  (samples, layout, scatter).  colour(means [n,3], dirs [n,3]) -> rgb [n,3] is asked for every (texel, direction) pair."""
  from tests import atlas_ref as A
  s = A.samples(m, c, filter)
  lay = A.layout(len(m['faces']), c)
  n, D = len(s['means']), len(dirs)
  rgb = colour(np.repeat(s['means'], D, 0), np.tile(np.asarray(dirs, F), (n, 1))).reshape(n, D, 3).astype(F)
  coef = fit(dirs, s['normals'], rgb, degree, lam)
  return A.scatter(lay, coef, s['face']).astype(F), A.uvs(len(m['faces']), lay), lay


def icosphere_mesh(subdivisions, radius=0.8):
  """The icosphere of tests/registration_ref.py as a host mesh dict with its unit normals: 80 faces at 1, 320 at 2."""
  from tests.registration_ref import icosphere
  v, f = icosphere(subdivisions)
  return dict(vertices=(radius * v).astype(F), normals=v.astype(F), faces=f.astype(np.int32))
