"""NumPy restatement of the mesh rasteriser's contract (include/mnerf.h, csrc/raster.hip): every face against every pixel, no
walks and no paths (the pixel box is one more clause of the coverage test, evaluated at every pixel), a lexicographic (depth bits,
face) minimum, then the shader.  float32 in the header's order: NumPy rounds
every product and sum to float32 and never contracts, so the kernels' buffers are held to these bit for bit."""

import numpy as np

EMPTY = np.uint64(0xffffffffffffffff)
F = np.float32


def homogeneous(verts, P):
  """h [V,3]: ((P[r,0] x + P[r,1] y) + P[r,2] z) + P[r,3]."""
  v, P = np.asarray(verts, F).reshape(-1, 3), np.asarray(P, F).reshape(3, 4)
  with np.errstate(all='ignore'):
    return np.stack([((P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2]) + P[r, 3] for r in range(3)], -1)


def cross(a, b):
  return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def setup(verts, faces, P, cull='none'):
  """dict(n [T,3,3] = s n_i, adet [T], s [T], h [T,3,3], ok [T]) of every face."""
  faces = np.asarray(faces, np.int64).reshape(-1, 3)
  V = len(np.asarray(verts).reshape(-1, 3))
  inside = ((faces >= 0) & (faces < V)).all(-1)
  hv = homogeneous(verts, P)
  with np.errstate(all='ignore'):
    h = hv[np.where(inside[:, None], faces, 0)] if V else np.zeros((len(faces), 3, 3), F)
    n = np.stack([cross(h[:, (i + 1) % 3], h[:, (i + 2) % 3]) for i in range(3)], 1)
    det = (n[:, 0, 0] * h[:, 0, 0] + n[:, 0, 1] * h[:, 0, 1]) + n[:, 0, 2] * h[:, 0, 2]
    ok = inside & np.isfinite(h).all((1, 2)) & np.isfinite(det) & (det != 0)
    s = np.where(det > 0, F(1), F(-1))
    if cull == 'back':
      ok &= ~(det > 0)
    return dict(n=s[:, None, None] * n, adet=np.abs(det), s=s, h=h, ok=ok)


def boxes(su, H, W):
  """(x0, x1, y0, y1) [T] float32, inclusive: the pixel box of every face: the projected corners' box widened by a pixel if all
  three h.z > 0, empty (x0 > x1) if all three h.z <= 0, else the whole image."""
  h = su['h']
  front, behind = (h[:, :, 2] > 0).all(-1), (h[:, :, 2] <= 0).all(-1)
  out = []
  with np.errstate(all='ignore'):
    for d, size in ((0, W), (1, H)):
      a = h[:, :, d] / h[:, :, 2]
      lo = np.maximum(np.floor(a.min(-1)) - F(1), F(0))
      hi = np.minimum(np.floor(a.max(-1)) + F(1), F(size - 1))
      out += [np.where(front, lo, np.where(behind, F(1), F(0))), np.where(front, hi, np.where(behind, F(0), F(size - 1)))]
  return out


def tie(n):
  a, b, c = n[..., 0], n[..., 1], n[..., 2]
  return (a > 0) | ((a == 0) & ((b > 0) | ((b == 0) & (c > 0))))


def edge_values(su, H, W, ids):
  """(E [n,3,H,W], S [n,H,W], zc [n,H,W], covered but for near [n,H,W]) of the faces `ids`."""
  px, py = (np.arange(W, dtype=F) + F(0.5))[None, None, None, :], (np.arange(H, dtype=F) + F(0.5))[None, None, :, None]
  n = su['n'][ids]
  with np.errstate(all='ignore'):
    E = (n[:, :, 0, None, None] * px + n[:, :, 1, None, None] * py) + n[:, :, 2, None, None]
    S = (E[:, 0] + E[:, 1]) + E[:, 2]
    zc = su['adet'][ids][:, None, None] / S
  inside = ((E > 0) | ((E == 0) & tie(n)[:, :, None, None])).all(1)
  x0, x1, y0, y1 = (b[ids][:, None, None] for b in boxes(su, H, W))
  xs, ys = np.arange(W, dtype=F)[None, None, :], np.arange(H, dtype=F)[None, :, None]
  inside &= (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
  return E, S, zc, inside & (S > 0) & np.isfinite(zc) & su['ok'][ids][:, None, None]


def visibility(verts, faces, P, H, W, near, cull='none', chunk=128, counts=False):
  """vis [H,W] uint64: min over the covering faces of (bits(zc) << 32) | face, all ones where there is none.  counts=True: also
  the number of faces that cover each pixel."""
  su = setup(verts, faces, P, cull)
  vis = np.full((H, W), EMPTY, dtype=np.uint64)
  cover = np.zeros((H, W), dtype=np.int64)
  T = len(su['ok'])
  for start in range(0, T, chunk):
    ids = np.arange(start, min(start + chunk, T))
    _, _, zc, cov = edge_values(su, H, W, ids)
    cov &= zc > F(near)
    key = (np.ascontiguousarray(zc).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)[:, None, None]
    vis = np.minimum(vis, np.where(cov, key, EMPTY).min(0))
    cover += cov.sum(0)
  return (vis, cover) if counts else vis


def _normalise(n):
  with np.errstate(all='ignore'):
    length = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    ok = (length > 0) & np.isfinite(length)
    return np.where(ok[..., None], n / np.where(ok, length, F(1))[..., None], F(0)), ok


def _blend(l, c):
  """(l_0 c_0 + l_1 c_1) + l_2 c_2 for l [n,3] and c [n,3,k]."""
  return (l[:, 0, None] * c[:, 0] + l[:, 1, None] * c[:, 1]) + l[:, 2, None] * c[:, 2]


def _image(t):
  t = np.asarray(t)
  return t.astype(F) / F(255) if t.dtype == np.uint8 else t.astype(F)


def shade(verts, normals, faces, P, vis, near, colors=None, texture=None, uv=None, bg=(1., 1., 1.)):
  """dict(face, depth, acc, bary, normals, rgb) of a visibility buffer, as mnr_raster_shade writes them."""
  verts, normals = np.asarray(verts, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
  faces = np.asarray(faces, np.int64).reshape(-1, 3)
  H, W = vis.shape
  su = setup(verts, faces, P)
  f = (vis & np.uint64(0xffffffff)).astype(np.int64)
  hit = (vis != EMPTY) & (f < len(faces))
  hit &= su['ok'][np.where(hit, f, 0)] if len(faces) else False
  out = dict(face=np.full((H, W), -1, np.int32), depth=np.zeros((H, W), F), acc=hit.astype(F), bary=np.zeros((H, W, 3), F),
             normals=np.zeros((H, W, 3), F), rgb=np.broadcast_to(np.asarray(bg, F), (H, W, 3)).copy())
  ys, xs = np.nonzero(hit)
  if len(ys) == 0:
    return out
  fi = f[ys, xs]
  n = su['n'][fi]
  px, py = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
  with np.errstate(all='ignore'):
    E = (n[:, :, 0] * px[:, None] + n[:, :, 1] * py[:, None]) + n[:, :, 2]
    S = (E[:, 0] + E[:, 1]) + E[:, 2]
    zc = su['adet'][fi] / S
    l = E / S[:, None]
    ids = faces[fi]
    nn, unit = _normalise(_blend(l, normals[ids]))
    v = verts[ids]
    g, gunit = _normalise(cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    nn = np.where(unit[:, None], nn, np.where(gunit[:, None], g, np.asarray([0, 0, 1], F)))
    if colors is not None:
      rgb = _blend(l, _image(colors)[ids])
    elif texture is not None:
      tex = _image(texture)
      Ht, Wt = tex.shape[:2]
      t = _blend(l, np.asarray(uv, F).reshape(-1, 3, 2)[fi])
      x, y = t[:, 0] * F(Wt) - F(0.5), (F(1) - t[:, 1]) * F(Ht) - F(0.5)
      xf, yf = np.floor(x), np.floor(y)
      fx, fy = (x - xf)[:, None], (y - yf)[:, None]
      xi = np.clip(np.nan_to_num(xf, nan=-1.), -1, Wt).astype(np.int64)
      yi = np.clip(np.nan_to_num(yf, nan=-1.), -1, Ht).astype(np.int64)
      xa, xb, ya, yb = np.clip(xi, 0, Wt - 1), np.clip(xi + 1, 0, Wt - 1), np.clip(yi, 0, Ht - 1), np.clip(yi + 1, 0, Ht - 1)
      top = (F(1) - fx) * tex[ya, xa] + fx * tex[ya, xb]
      bot = (F(1) - fx) * tex[yb, xa] + fx * tex[yb, xb]
      rgb = (F(1) - fy) * top + fy * bot
    else:
      rgb = F(0.5) + F(0.5) * nn
  out['face'][ys, xs], out['depth'][ys, xs], out['bary'][ys, xs], out['normals'][ys, xs], out['rgb'][ys, xs] = fi, zc, l, nn, rgb
  return out


def render(m, P, H, W, near, cull='none', **kw):
  vis = visibility(m['vertices'], m['faces'], P, H, W, near, cull)
  out = shade(m['vertices'], m['normals'], m['faces'], P, vis, near, **kw)
  out['vis'] = vis
  return out


def projected_vertices(verts, P):
  """[V,2] float64 pixel positions of the vertices in front of the camera plane (NaN for the others)."""
  v, P = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(P, np.float64).reshape(3, 4)
  h = v @ P[:, :3].T + P[:, 3]
  with np.errstate(all='ignore'):
    return np.where(h[:, 2:] > 0, h[:, :2] / h[:, 2:], np.nan)


def vertex_clearance(verts, P):
  """The smallest distance (pixels, max norm) of a projected vertex from a pixel centre: the tests' precondition is >= 1e-3."""
  uv = projected_vertices(verts, P)
  uv = uv[np.isfinite(uv).all(-1)]
  if len(uv) == 0:
    return np.inf
  d = np.abs(uv - (np.floor(uv) + 0.5)).max(-1)
  return float(d.min())


def latlong_sphere(bands=12, radius=1.0):
  """A closed latitude-longitude sphere: `bands` latitude bands, 2 `bands` meridians, two pole vertices; faces counter-clockwise
  seen from outside, unit normals.  bands = 12: 266 vertices, 528 faces."""
  nlat, nlon = bands, 2 * bands
  th = np.pi * np.arange(1, nlat) / nlat
  ph = 2 * np.pi * np.arange(nlon) / nlon
  ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph), np.cos(th)[:, None] * np.ones_like(ph)], -1)
  verts = np.concatenate([[[0, 0, 1.]], ring.reshape(-1, 3), [[0, 0, -1.]]])
  idx = lambda i, j: 1 + i * nlon + (j % nlon)
  south = len(verts) - 1
  faces = []
  for j in range(nlon):
    faces.append((0, idx(0, j), idx(0, j + 1)))
    for i in range(nlat - 2):
      faces += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    faces.append((south, idx(nlat - 2, j + 1), idx(nlat - 2, j)))
  return dict(vertices=(radius * verts).astype(F), normals=verts.astype(F), faces=np.asarray(faces, np.int32))


def look_at(eye, target=(0., 0., 0.), up=(0., 0., 1.)):
  """camtoworld [3,4] in the OpenGL convention of the datasets (columns right, up, -forward, position)."""
  eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
  fwd = (target - eye) / np.linalg.norm(target - eye)
  right = np.cross(fwd, np.asarray(up, np.float64))
  right /= np.linalg.norm(right)
  return np.stack([right, np.cross(right, fwd), -fwd, eye], -1)


def pixtocam(focal, W, H):
  return np.linalg.inv(np.array([[focal, 0, W / 2.], [0, focal, H / 2.], [0, 0, 1.]]))
