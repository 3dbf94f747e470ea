"""NumPy restatement of csrc/meshclean.hip's two contracts (include/mnerf.h), written for clarity.

Components: host union-find.  Clustering: float32 keys in the header's operation order, float64 sums in the header's order
(np.add.at adds its operands one after the other in index order, and the lists are sorted stably, so a cluster's terms arrive
in ascending id), the same closed-form cofactor solve spelled out element-wise (no np.linalg).  `quadric_error` evaluates
E(x) of a cluster directly from its faces, independently of A and r.
"""

import numpy as np

QEM_REG = 1e-3
CELL_LIMIT = 1 << 21


# ---- connected components

def components(faces, n_verts):
  """labels [V] int32: the smallest vertex id each vertex is connected to through face edges."""
  parent = list(range(int(n_verts)))

  def find(x):
    while parent[x] != x:
      parent[x] = parent[parent[x]]
      x = parent[x]
    return x

  for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
    for u, v in ((a, b), (b, c)):
      ru, rv = find(u), find(v)
      if ru != rv:
        parent[max(ru, rv)] = min(ru, rv)                  # the root is always the smallest id of its tree
  return np.array([find(v) for v in range(int(n_verts))], np.int32).reshape(-1)


def compact(m, keep_faces):
  verts, faces = np.asarray(m['vertices']), np.asarray(m['faces']).reshape(-1, 3)
  faces = faces[keep_faces]
  used = np.zeros((len(verts),), bool)
  used[faces.reshape(-1)] = True
  new_id = (np.cumsum(used) - 1).astype(np.int32)
  colors = m.get('colors')
  return dict(vertices=verts[used], normals=np.asarray(m['normals'])[used], faces=new_id[faces].reshape(-1, 3),
              colors=None if colors is None else np.asarray(colors)[used])


def component_face_counts(faces, labels):
  """{label: faces} of the components that have faces."""
  ids, counts = np.unique(labels[np.asarray(faces).reshape(-1, 3)[:, 0]], return_counts=True)
  return dict(zip(ids.tolist(), counts.tolist()))


def filter_components(m, min_faces=0, keep_largest=0):
  faces = np.asarray(m['faces']).reshape(-1, 3)
  labels = components(faces, len(m['vertices']))
  counts = component_face_counts(faces, labels)
  kept = [l for l, n in counts.items() if n >= min_faces]
  if keep_largest > 0:
    best = sorted(counts, key=lambda l: (-counts[l], l))[:keep_largest]
    kept = [l for l in kept if l in best]
  return compact(m, np.isin(labels[faces[:, 0]], kept) if len(faces) else np.zeros((0,), bool))


# ---- vertex clustering

def cluster_keys(verts, origin, cell):
  v, o, cell = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(origin, np.float32), np.float32(cell)
  assert np.isfinite(v).all()
  q = np.floor((v - o) / cell)
  assert q.dtype == np.float32 and (q >= 0).all() and (q < CELL_LIMIT).all()
  c = q.astype(np.int64)
  return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def cell_centres(ukeys, origin, cell):
  c = np.stack([(ukeys >> 42) & 0x1fffff, (ukeys >> 21) & 0x1fffff, ukeys & 0x1fffff], -1).astype(np.float64)
  return np.asarray(origin, np.float32).astype(np.float64) + np.float64(np.float32(cell)) * (c + 0.5)


def face_lists(faces, vmap, K):
  """(cluster of each list entry, its face id): every cluster a face touches, once, by cluster then ascending face id."""
  mapped = vmap[faces]                                                            # [T,3]
  inc = mapped.copy()
  inc[:, 1] = np.where(mapped[:, 1] != mapped[:, 0], mapped[:, 1], -1)
  inc[:, 2] = np.where((mapped[:, 2] != mapped[:, 0]) & (mapped[:, 2] != mapped[:, 1]), mapped[:, 2], -1)
  flat = inc.reshape(-1)
  at = np.nonzero(flat >= 0)[0]
  order = np.argsort(flat[at], kind='stable')
  return flat[at][order], at[order] // 3


def face_terms(verts, faces, centre):
  """(n [.,3], L [.], d [.], p_a [.,3]) of faces relative to a centre [.,3] (or [3]), float64, in the header's order."""
  v = np.asarray(verts, np.float32).astype(np.float64)
  pa, pb, pc = (v[faces[:, s]] - centre for s in range(3))
  e1, e2 = pb - pa, pc - pa
  n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
  L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
  d = (n[:, 0] * pa[:, 0] + n[:, 1] * pa[:, 1]) + n[:, 2] * pa[:, 2]
  return n, L, d, pa


def simplify(m, cell, origin=None):
  """-> dict(vertices, normals, faces, colors, map, fallback, x [K,3] float64 the solved points and g [K,3] the centroids (both
  relative to the cell centres), centres [K,3], trace [K])."""
  verts = np.asarray(m['vertices'], np.float32).reshape(-1, 3)
  normals = np.asarray(m['normals'], np.float32).reshape(-1, 3)
  faces = np.asarray(m['faces'], np.int32).reshape(-1, 3)
  colors = m.get('colors')
  cell = np.float32(cell)
  V, T = len(verts), len(faces)
  if V == 0:
    return dict(vertices=verts, normals=normals, faces=np.zeros((0, 3), np.int32), colors=colors, map=np.zeros((0,), np.int32),
                fallback=np.zeros((0,), bool))
  origin = verts.min(0) if origin is None else np.asarray(origin, np.float32)
  keys = cluster_keys(verts, origin, cell)
  ukeys, vmap = np.unique(keys, return_inverse=True)
  vmap = vmap.reshape(-1)
  K = len(ukeys)
  centres = cell_centres(ukeys, origin, cell)

  members = np.argsort(vmap, kind='stable')
  of_member = vmap[members]
  count = np.bincount(vmap, minlength=K)
  sg, sn = np.zeros((K, 3)), np.zeros((K, 3))
  np.add.at(sg, of_member, verts[members].astype(np.float64) - centres[of_member])
  np.add.at(sn, of_member, normals[members].astype(np.float64))
  g = sg / count[:, None].astype(np.float64)

  of_entry, face = face_lists(faces, vmap, K)
  n, L, d, _ = face_terms(verts, faces[face], centres[of_entry])
  with np.errstate(all='ignore'):
    ok = (L > 0) & (L < np.inf)
  n, L, d, of_ok = n[ok], L[ok], d[ok], of_entry[ok]
  A = {ij: np.zeros((K,)) for ij in ('00', '01', '02', '11', '12', '22')}
  for ij in A:
    np.add.at(A[ij], of_ok, (n[:, int(ij[0])] * n[:, int(ij[1])]) / L)
  r = np.zeros((K, 3))
  for i in range(3):
    np.add.at(r[:, i], of_ok, (n[:, i] * d) / L)

  tr = (A['00'] + A['11']) + A['22']
  lam = (QEM_REG * tr) / 3.0
  M00, M11, M22, M01, M02, M12 = A['00'] + lam, A['11'] + lam, A['22'] + lam, A['01'], A['02'], A['12']
  b0, b1, b2 = r[:, 0] + lam * g[:, 0], r[:, 1] + lam * g[:, 1], r[:, 2] + lam * g[:, 2]
  c00, c01, c02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
  c11, c12, c22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
  det = (M00 * c00 + M01 * c01) + M02 * c02
  with np.errstate(all='ignore'):
    x = np.stack([((c00 * b0 + c01 * b1) + c02 * b2) / det, ((c01 * b0 + c11 * b1) + c12 * b2) / det,
                  ((c02 * b0 + c12 * b1) + c22 * b2) / det], -1)
    half = np.float64(cell) / 2.0
    take = (tr > 0) & np.isfinite(x).all(-1) & (np.abs(x) <= half).all(-1)
    out_v = (centres + np.where(take[:, None], x, g)).astype(np.float32)
    length = np.sqrt((sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1]) + sn[:, 2] * sn[:, 2])
    unit = (length > 0) & (length < np.inf)
    out_n = np.where(unit[:, None], sn / np.where(unit, length, 1.)[:, None], 0.).astype(np.float32)
  out_c = None
  if colors is not None:
    sc = np.zeros((K, 3), np.int64)
    np.add.at(sc, vmap, np.asarray(colors).reshape(-1, 3).astype(np.int64))
    out_c = ((2 * sc + count[:, None]) // (2 * count[:, None])).astype(np.uint8)

  mapped = vmap[faces].astype(np.int32)
  distinct = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])
  seen, keep = set(), np.zeros((T,), bool)
  for f in np.nonzero(distinct)[0].tolist():
    t = mapped[f].tolist()
    s = t.index(min(t))
    t = tuple(t[s:] + t[:s])
    if t not in seen:
      seen.add(t)
      keep[f] = True
  return dict(vertices=out_v, normals=out_n, faces=mapped[keep].reshape(-1, 3), colors=out_c, map=vmap.astype(np.int32), fallback=~take,
              x=x, g=g, centres=centres, trace=tr)


def quadric_error(verts, faces, vmap, k, centre, x):
  """E(x) = sum over the faces that touch cluster k (each once, degenerate ones skipped) of L (n / L . (x - p_a))^2, float64, with
  x and p_a relative to `centre` [3]."""
  faces = np.asarray(faces).reshape(-1, 3)
  touch = (vmap[faces] == k).any(-1)
  n, L, d, pa = face_terms(verts, faces[touch], np.asarray(centre, np.float64))
  ok = (L > 0) & (L < np.inf)
  n, L, pa = n[ok], L[ok], pa[ok]
  dist = ((n / L[:, None]) * (np.asarray(x, np.float64) - pa)).sum(-1)
  return float((L * dist * dist).sum())


def cluster_errors(verts, faces, vmap, centres, x):
  """[K] E(x_k) for every cluster, x [K,3] relative to centres [K,3] (one pass over the face lists)."""
  faces = np.asarray(faces).reshape(-1, 3)
  K = len(centres)
  of_entry, face = face_lists(faces, vmap, K)
  n, L, d, pa = face_terms(verts, faces[face], centres[of_entry])
  with np.errstate(all='ignore'):
    ok = (L > 0) & (L < np.inf)
    dist = ((n / L[:, None]) * (np.asarray(x, np.float64)[of_entry] - pa)).sum(-1)
    term = np.where(ok, L * dist * dist, 0.)
  return np.bincount(of_entry, weights=term, minlength=K)


def boundary_margin(ref, cell):
  """The smallest distance, over every cluster with a finite solve and every axis, of |x_a| from cell / 2, in units of cell."""
  x = ref['x'][np.isfinite(ref['x']).all(-1) & (ref['trace'] > 0)]
  if len(x) == 0:
    return np.inf
  return float(np.abs(np.abs(x) - np.float64(np.float32(cell)) / 2.0).min() / np.float64(np.float32(cell)))


# ---- the meshes the tests share

def strip(n_verts, seed, drop=()):
  """A triangle strip over n_verts vertices (face i = (i, i+1, i+2), odd ones flipped), the faces in `drop` removed, and the
  vertex ids permuted with a fixed seed: -> (faces [T,3] int32, the permutation)."""
  i = np.arange(n_verts - 2)
  f = np.stack([i, np.where(i % 2 == 0, i + 1, i + 2), np.where(i % 2 == 0, i + 2, i + 1)], -1)
  f = np.delete(f, list(drop), axis=0)
  perm = np.random.default_rng(seed).permutation(n_verts)
  return perm[f].astype(np.int32), perm


def concat(meshes):
  """The union of mesh dicts, indices offset."""
  off, parts = 0, []
  for m in meshes:
    parts.append(np.asarray(m['faces']) + off)
    off += len(m['vertices'])
  cols = [m.get('colors') for m in meshes]
  return dict(vertices=np.concatenate([m['vertices'] for m in meshes]), normals=np.concatenate([m['normals'] for m in meshes]),
              faces=np.concatenate(parts).astype(np.int32), colors=None if any(c is None for c in cols) else np.concatenate(cols))


def permute_vertices(m, seed):
  """The same mesh with vertex ids permuted (new id = perm[old id]); face order unchanged."""
  V = len(m['vertices'])
  perm = np.random.default_rng(seed).permutation(V)
  inv = np.argsort(perm)
  colors = m.get('colors')
  return dict(vertices=m['vertices'][inv], normals=m['normals'][inv], faces=perm[m['faces']].astype(np.int32),
              colors=None if colors is None else colors[inv])


def planar_patch(n=24, z=0.3, seed=7):
  """A jittered n x n triangulated grid in the plane z = const (spacing 1 / (n - 1), jitter 30 % of it)."""
  rng = np.random.default_rng(seed)
  i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
  h = 1. / (n - 1)
  xy = np.stack([i, j], -1).reshape(-1, 2) * h + rng.uniform(-0.3, 0.3, (n * n, 2)) * h
  verts = np.concatenate([xy, np.full((n * n, 1), z)], -1).astype(np.float32)
  q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
  faces = np.concatenate([np.stack([q, q + n, q + n + 1], -1), np.stack([q, q + n + 1, q + 1], -1)]).astype(np.int32)
  normals = np.tile(np.array([[0., 0., 1.]], np.float32), (n * n, 1))
  return dict(vertices=verts, normals=normals, faces=faces, colors=None), h


def corner_patch(n=5, corner=(0.52, 0.47, 0.55), size=0.4):
  """Three mutually orthogonal square patches (n x n vertices each, side `size`) that meet at `corner`, as separate sheets: with
  origin (0, 0, 0) and cell 1 everything lies in one cell, whose quadric has full rank and its minimum at the corner."""
  c = np.array(corner)
  t = np.linspace(0., size, n)
  u, v = np.meshgrid(t, t, indexing='ij')
  verts, faces, normals = [], [], []
  for axis in range(3):
    a, b = (axis + 1) % 3, (axis + 2) % 3
    p = np.tile(c, (n * n, 1))
    p[:, a] += u.reshape(-1)
    p[:, b] += v.reshape(-1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij')
    q = (i * n + j).reshape(-1) + axis * n * n
    faces += [np.stack([q, q + n, q + n + 1], -1), np.stack([q, q + n + 1, q + 1], -1)]
    verts.append(p)
    nn = np.zeros((n * n, 3))
    nn[:, axis] = 1.
    normals.append(nn)
  return dict(vertices=np.concatenate(verts).astype(np.float32), normals=np.concatenate(normals).astype(np.float32),
              faces=np.concatenate(faces).astype(np.int32), colors=None), c


# ---- the marching-tetrahedra meshes and the (mesh, cell, origin) cases of the simplification tests (computed once, never written to)

import functools

from tests import mesh_ref as R

# name -> (field, level, origin, spacing)
SOURCES = {
    'sphere': lambda: (R.sphere_field(), 0., R.ORIGIN, R.H),
    'torus': lambda: (R.torus_field(), 0., R.ORIGIN, R.H),
    'noise': lambda: (R.noise_field(), 0.5, (0., 0., 0.), 1.),
    'noise1': lambda: (R.noise_field(), 1.0, (0., 0., 0.), 1.),
}
CELL_FACTORS = (2., 3.7)
SIMPLIFY_MESHES = ('sphere', 'torus', 'noise')


@functools.lru_cache(maxsize=None)
def source_mesh(name):
  """(mesh dict with random uint8 colours, grid spacing) of SOURCES[name]."""
  field, level, origin, spacing = SOURCES[name]()
  verts, normals, faces = R.marching_tetrahedra(field.astype(np.float32), level, origin, spacing)
  colors = np.random.default_rng(len(verts)).integers(0, 256, (len(verts), 3)).astype(np.uint8)
  for a in (verts, normals, faces, colors):
    a.setflags(write=False)
  return dict(vertices=verts, normals=normals, faces=faces, colors=colors), spacing


def explicit_origin(m, cell):
  """An origin below the mesh that is no multiple of the cell away from its corner."""
  return (m['vertices'].min(0).astype(np.float64) - np.array([0.37, 0.11, 0.23]) * cell).astype(np.float32)


@functools.lru_cache(maxsize=None)
def simplify_case(name, factor, explicit):
  """(mesh, cell, origin or None, the restatement's result)."""
  m, h = source_mesh(name)
  cell = float(np.float32(factor * h))
  origin = tuple(explicit_origin(m, cell).tolist()) if explicit else None
  ref = simplify(m, cell, origin)
  for a in ref.values():
    if a is not None:
      a.setflags(write=False)
  return m, cell, origin, ref


SIMPLIFY_CASES = [(name, factor, explicit) for name in SIMPLIFY_MESHES for factor in CELL_FACTORS for explicit in (False, True)]


def shortest_edge(m):
  v, f = np.asarray(m['vertices'], np.float64), np.asarray(m['faces'])
  e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
  return float(np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1).min())
