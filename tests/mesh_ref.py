"""NumPy restatement of csrc/mesh.hip (marching tetrahedra on the Kuhn decomposition of a regular grid), written for clarity.

Same grid convention, vertex order and face order as the kernels; positions in float32 in the kernels' operation order, so
they are reproduced bit for bit.  What is NOT restated is the kernels' winding rule (the parity of the permutation and of the
sign pattern): here every triangle is oriented geometrically, flipped if its normal points toward an inside corner of its
tetrahedron, which makes this an independent check of that rule.
"""

import itertools
import math

import numpy as np

DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = list(itertools.permutations(range(3)))            # lexicographic


def gradient(f, spacing):
  """[nx,ny,nz,3] float32: (f[hi] - f[lo]) / (spacing * (hi - lo)) per axis, hi / lo the neighbours clipped to the grid."""
  f = np.asarray(f, np.float32)
  g = np.zeros(f.shape + (3,), np.float32)
  with np.errstate(all='ignore'):
    for d in range(3):
      idx = np.arange(f.shape[d])
      lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, f.shape[d] - 1)
      shape = [1, 1, 1]
      shape[d] = -1
      den = np.float32(spacing) * (hi - lo).astype(np.float32).reshape(shape)
      g[..., d] = (np.take(f, hi, axis=d) - np.take(f, lo, axis=d)) / den
  return g


def marching_tetrahedra(field, level, origin, spacing):
  """-> (verts [V,3] float32, normals [V,3] float32, faces [T,3] int32)."""
  f = np.asarray(field, np.float32)
  nx, ny, nz = f.shape
  level, spacing = np.float32(level), np.float32(spacing)
  origin = np.asarray(origin, np.float32)
  with np.errstate(invalid='ignore'):
    inside = f >= level                                                          # NaN: outside

  # ---- vertices: by lower end (linear order), then by direction
  carries = np.zeros((nx, ny, nz, 7), bool)
  for e, (dx, dy, dz) in enumerate(DIRS):
    lo = inside[:nx - dx, :ny - dy, :nz - dz]
    carries[:nx - dx, :ny - dy, :nz - dz, e] = lo != inside[dx:, dy:, dz:]
  keys = np.argwhere(carries)                                                    # rows (i, j, k, e), lexicographic
  vid = {tuple(int(x) for x in key): n for n, key in enumerate(keys)}
  lower = keys[:, :3]
  upper = lower + np.array(DIRS)[keys[:, 3]]
  f0, f1 = f[tuple(lower.T)], f[tuple(upper.T)]
  with np.errstate(all='ignore'):
    t = (level - f0) / (f1 - f0)
    t = np.where((t >= 0) & (t <= 1), t, np.float32(0.5)).astype(np.float32)[:, None]
    P0 = origin + spacing * lower.astype(np.float32)
    P1 = origin + spacing * upper.astype(np.float32)
    verts = P0 + t * (P1 - P0)
    grad = gradient(f, spacing)
    g0, g1 = grad[tuple(lower.T)], grad[tuple(upper.T)]
    g = g0 + t * (g1 - g0)
    length = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])[:, None]
    ok = (length > 0) & np.isfinite(length)
    normals = np.where(ok, -g / np.where(ok, length, np.float32(1)), np.float32(0))
  assert verts.dtype == np.float32 and normals.dtype == np.float32

  # ---- faces: by cell (linear order), then tetrahedron, then triangle
  def vertex(c0, c1):
    """(id, midpoint in index space) of the vertex on the tetrahedron edge between corners c0 and c1"""
    lo, hi = (c0, c1) if sum(c0) < sum(c1) else (c1, c0)
    e = DIRS.index(tuple(h - l for l, h in zip(lo, hi)))
    return vid[lo + (e,)], (np.array(lo, float) + np.array(hi, float)) / 2

  corners_in = sum(inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(int) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1))
  faces = []
  for cell in np.argwhere((corners_in > 0) & (corners_in < 8)):
    p = tuple(int(x) for x in cell)
    for perm in PERMS:
      path = [p]
      for axis in perm:
        q = list(path[-1])
        q[axis] += 1
        path.append(tuple(q))
      ins = [bool(inside[c]) for c in path]
      n_in = sum(ins)
      if n_in in (0, 4):
        continue
      if n_in in (1, 3):
        lone = ins.index(n_in == 1)
        tris = [[vertex(path[lone], path[o]) for o in range(4) if o != lone]]
      else:
        a, b = [r for r in range(4) if ins[r]]
        c, d = [r for r in range(4) if not ins[r]]
        quad = [vertex(path[a], path[c]), vertex(path[a], path[d]), vertex(path[b], path[d]), vertex(path[b], path[c])]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
      an_inside_corner = np.array(path[ins.index(True)], float)
      for tri in tris:
        (i0, m0), (i1, m1), (i2, m2) = tri
        # geometric orientation, on the edges' midpoints (the true vertices may coincide where the field equals the level)
        toward_inside = np.dot(np.cross(m1 - m0, m2 - m0), an_inside_corner - m0) > 0
        faces.append([i0, i2, i1] if toward_inside else [i0, i1, i2])
  return verts, normals, np.array(faces, np.int32).reshape(-1, 3)


def canonical_faces(faces):
  """The faces, each rotated so that its smallest index comes first, sorted: equal iff the oriented face sets are equal."""
  f = np.asarray(faces).reshape(-1, 3)
  k = np.argmin(f, axis=1)
  rolled = np.stack([f[np.arange(len(f)), (k + s) % 3] for s in range(3)], -1) if len(f) else f
  return rolled[np.lexsort(rolled.T[::-1])] if len(f) else rolled


def directed_edges_once(faces):
  """Every directed edge of the mesh occurs exactly once (with closedness: a consistently oriented surface)."""
  f = np.asarray(faces).reshape(-1, 3)
  e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
  return len(np.unique(e, axis=0)) == len(e)


# ---- the fields the tests share

SHAPE = (29, 31, 33)
H = 2. / 32
ORIGIN = (-14 * H + 0.013, -15 * H - 0.02, -1 + 0.007)


def grid_xyz(shape=SHAPE, origin=ORIGIN, spacing=H):
  i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
  return origin[0] + spacing * i, origin[1] + spacing * j, origin[2] + spacing * k


def sphere_field():
  x, y, z = grid_xyz()
  return 0.6 - np.sqrt(x * x + y * y + z * z)


def torus_field():
  x, y, z = grid_xyz()
  return 0.2 - np.sqrt((np.sqrt(y * y + z * z) - 0.55) ** 2 + x * x)


def noise_field():
  return np.pad(np.random.default_rng(0).standard_normal((7, 9, 10)), 1, constant_values=-5.)


def sphere_bounds(verts, stats, h=H):
  """What a marching-tetrahedra mesh of f = 0.6 - |x| at spacing h satisfies: it is inscribed and its volume is within 2 % of the
  ball's; every vertex is within the linear-interpolation bound of |x| over an edge of length <= sqrt(3) h of the sphere."""
  ratio = stats['signed_volume'] / (4. / 3. * math.pi * 0.6 ** 3)
  dev = np.abs(np.linalg.norm(np.asarray(verts, np.float64), axis=1) - 0.6).max()
  bound = 3 * h * h / (8 * (0.6 - math.sqrt(3) * h))
  print(f'sphere: volume ratio {ratio:.4f}, max ||v| - 0.6| {dev:.3e} (bound {bound:.3e})')
  assert 0.98 <= ratio <= 1.0
  assert dev <= bound
  assert stats['boundary_edges'] == 0 and stats['nonmanifold_edges'] == 0 and stats['euler'] == 2
