"""NumPy restatement of the texture atlas contract of include/mnerf.h (csrc/atlas.hip), written for clarity: it walks the cells
and the face-local texels of the two faces of a cell, never a linear sample index, and takes the UV corners from the contract's
table as it is printed.  float32 where the contract says float32, in the order written (NumPy does not contract).

  layout            (cell, cols, rows, W, H, n_samples) of T faces
  samples           means, covs, normals, viewdirs, face in sample order s = cell c (c + 1) + Y (c + 1) + X
  uvs               [T,3,2]
  store             texture, mask and the float texture from per-sample colours (scatter: any per-sample values, float64)
  sample_bilinear   a clamp-to-edge bilinear lookup with texel centres at + 0.5, float64 (sample_bilinear_px: at pixel positions)
"""

import math

import numpy as np

f32 = np.float32
MIN_CELL = 3


def layout(T, c, cols=None):
  assert c >= MIN_CELL and T >= 0
  ncells = (T + 1) // 2
  if cols is None:
    cols = max(1, math.ceil(math.sqrt(ncells * c / (c + 1))))
  rows = math.ceil(ncells / cols)
  return dict(cell=c, cols=cols, rows=rows, W=cols * (c + 1) if ncells else 0, H=rows * c, n_samples=ncells * c * (c + 1))


def local_texels(c):
  """[(half, x', y', X, Y)] of a cell: the face-local texels x' + y' <= c - 1 of the lower (half 0) and the upper face (half 1) with
  the cell-local texel each of them is."""
  out = []
  for yl in range(c):
    for xl in range(c - yl):
      out.append((0, xl, yl, xl, yl))
      out.append((1, xl, yl, c - xl, c - 1 - yl))
  return out


def _unit(n):
  """(n / |n| in float32, where 0 < |n| < inf)."""
  length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
  good = (length > 0) & np.isfinite(length)
  return n / np.where(good, length, f32(1))[:, None], good


def samples(m, c, filter=1.0):
  """dict(means [n,3], covs [n,3,3], normals [n,3], viewdirs [n,3] float32, face [n] int32), n = ceil(T / 2) c (c + 1)."""
  verts, normals, faces = (np.asarray(m[k]) for k in ('vertices', 'normals', 'faces'))
  T = len(faces)
  ncells = (T + 1) // 2
  den, cov_scale, up = f32(c - 2), f32(filter * filter / 12.), np.array([0., 0., 1.], f32)
  means = np.zeros((ncells, c, c + 1, 3), f32)
  covs = np.zeros((ncells, c, c + 1, 3, 3), f32)
  nrm = np.broadcast_to(up, (ncells, c, c + 1, 3)).copy()
  view = nrm.copy()
  face = np.full((ncells, c, c + 1), -1, np.int32)
  with np.errstate(all='ignore'):
    for half in (0, 1):
      ids = np.arange(half, T, 2)                             # face 2k + half lives in cell k
      k = np.arange(len(ids))
      v, vn = verts[faces[ids]].astype(f32), normals[faces[ids]].astype(f32)          # [m, corner, xyz]
      e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
      a, b = e1 / den, e2 / den
      cov = cov_scale * (a[:, :, None] * a[:, None, :] + b[:, :, None] * b[:, None, :])
      g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                    e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
      g_unit, g_good = _unit(g)
      face_ok = np.isfinite(v).all((1, 2)) & np.isfinite(cov).all((1, 2))
      for h, xl, yl, X, Y in local_texels(c):
        if h != half:
          continue
        b1, b2 = f32(xl) / den, f32(yl) / den
        b0 = (f32(1) - b1) - b2
        p = (b0 * v[:, 0] + b1 * v[:, 1]) + b2 * v[:, 2]
        ok = face_ok & np.isfinite(p).all(1)
        n_unit, n_good = _unit((b0 * vn[:, 0] + b1 * vn[:, 1]) + b2 * vn[:, 2])
        n = np.where(n_good[:, None], n_unit, np.where(g_good[:, None], g_unit, up))
        d = np.where((n_good | g_good)[:, None], -n, up)
        kk = k[ok]
        means[kk, Y, X], covs[kk, Y, X], nrm[kk, Y, X], view[kk, Y, X], face[kk, Y, X] = p[ok], cov[ok], n[ok], d[ok], ids[ok]
  return dict(means=means.reshape(-1, 3), covs=covs.reshape(-1, 3, 3), normals=nrm.reshape(-1, 3), viewdirs=view.reshape(-1, 3),
              face=face.reshape(-1))


def uvs(T, lay):
  """uv [T,3,2] float32: the contract's table, u = px / float(W), v = 1 - py / float(H)."""
  c, cols, W, H = lay['cell'], lay['cols'], lay['W'], lay['H']
  uv = np.zeros((T, 3, 2), f32)
  for k in range((T + 1) // 2):
    X0, Y0 = (k % cols) * (c + 1), (k // cols) * c
    table = {0: ((X0 + .5, Y0 + .5), (X0 + c - 1.5, Y0 + .5), (X0 + .5, Y0 + c - 1.5)),
             1: ((X0 + c + .5, Y0 + c - .5), (X0 + 2.5, Y0 + c - .5), (X0 + c + .5, Y0 + 1.5))}
    for half in (0, 1):
      if 2 * k + half < T:
        for corner, (px, py) in enumerate(table[half]):
          uv[2 * k + half, corner] = f32(px) / f32(W), f32(1) - f32(py) / f32(H)
  return uv


def quantise(rgb):
  rgb = np.asarray(rgb, f32)
  q = np.floor(np.clip(np.where(np.isnan(rgb), f32(0), rgb), f32(0), f32(1)) * f32(255) + f32(0.5))
  return q.astype(np.uint8)


def store(lay, rgb, face):
  """(texture [H,W,3] uint8, mask [H,W] uint8, texture_f32 [H,W,3] float32) of per-sample colours rgb [n,3] and owners face [n]."""
  c, cols, W, H = lay['cell'], lay['cols'], lay['W'], lay['H']
  ncells = lay['n_samples'] // (c * (c + 1)) if lay['n_samples'] else 0
  rgb = np.asarray(rgb, f32).reshape(ncells, c, c + 1, 3)
  face = np.asarray(face).reshape(ncells, c, c + 1)
  texture, mask, tex_f = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), np.zeros((H, W, 3), f32)
  q = quantise(rgb)
  for k in range(ncells):
    X0, Y0 = (k % cols) * (c + 1), (k // cols) * c
    own = face[k] >= 0                                      # [c, c + 1]: the cell's texels that have a sample
    texture[Y0:Y0 + c, X0:X0 + c + 1][own] = q[k][own]
    mask[Y0:Y0 + c, X0:X0 + c + 1][own] = 255
    tex_f[Y0:Y0 + c, X0:X0 + c + 1][own] = rgb[k][own]
  return texture, mask, tex_f


def scatter(lay, values, face):
  """values [n, ...] of the samples as an image [H, W, ...] float64: every sample with face >= 0 at its own texel, 0 elsewhere."""
  c, cols, W, H = lay['cell'], lay['cols'], lay['W'], lay['H']
  ncells = lay['n_samples'] // (c * (c + 1)) if lay['n_samples'] else 0
  values = np.asarray(values, np.float64)
  tail = values.shape[1:]
  values, face = values.reshape((ncells, c, c + 1) + tail), np.asarray(face).reshape(ncells, c, c + 1)
  image = np.zeros((H, W) + tail, np.float64)
  for k in range(ncells):
    X0, Y0 = (k % cols) * (c + 1), (k // cols) * c
    block = image[Y0:Y0 + c, X0:X0 + c + 1]
    block[face[k] >= 0] = values[k][face[k] >= 0]
  return image


def sample_bilinear_px(texture, px, py):
  """Bilinear lookup of texture [H,W,...] at pixel positions (px to the right, py down from the top edge; texel (X, Y) has its
  centre at (X + .5, Y + .5)), clamp-to-edge, float64, as two nested lerps a + f (b - a): four equal texels return that value
  exactly, and a texel with weight 0 contributes exactly nothing."""
  tex = np.asarray(texture, np.float64)
  H, W = tex.shape[:2]
  x, y = np.asarray(px, np.float64) - .5, np.asarray(py, np.float64) - .5
  i, j = np.floor(x), np.floor(y)
  fx, fy = (x - i).reshape(x.shape + (1,) * (tex.ndim - 2)), (y - j).reshape(y.shape + (1,) * (tex.ndim - 2))
  i0, i1 = np.clip(i, 0, W - 1).astype(np.int64), np.clip(i + 1, 0, W - 1).astype(np.int64)
  j0, j1 = np.clip(j, 0, H - 1).astype(np.int64), np.clip(j + 1, 0, H - 1).astype(np.int64)
  top = tex[j0, i0] + fx * (tex[j0, i1] - tex[j0, i0])
  bottom = tex[j1, i0] + fx * (tex[j1, i1] - tex[j1, i0])
  return top + fy * (bottom - top)


def sample_bilinear(texture, uv):
  """sample_bilinear_px at px = u W, py = (1 - v) H for uv [..., 2] (float64 arithmetic)."""
  uv = np.asarray(uv, np.float64)
  H, W = np.asarray(texture).shape[:2]
  return sample_bilinear_px(texture, uv[..., 0] * W, (1. - uv[..., 1]) * H)
