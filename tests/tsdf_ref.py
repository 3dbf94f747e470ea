"""NumPy restatement of csrc/tsdf.hip, written for clarity: the seven steps of mnr_tsdf_integrate (include/mnerf.h) in float32
in the kernel's operation order, vectorised over the voxels, so that the volumes are reproduced bit for bit; the validity
filter of ops.marching_tetrahedra(valid=...) by enumerating the grid edges as tests/mesh_ref.py does; TsdfVolume.mesh on top of
both; and the analytic sphere scene the tests share.

What is NOT restated: the brick mapping and the per-brick culling of frames.  Every frame is looked at for every voxel here, so
bit-equality with the kernel is also the proof that culling changes nothing.
"""

import functools
import math

import numpy as np

from tests import mesh_ref as R

F32 = np.float32
MAX_FRAMES = 64                                              # MNR_TSDF_MAX_FRAMES: a longer stack is folded 64 frames at a time


def integrate(tsdf, weight, color, origin, spacing, trunc, proj, depth, acc=None, rgb=None, acc_threshold=0.5, stats=None):
  """Updates tsdf, weight [nx,ny,nz] and color [nx,ny,nz,3] (or None) in place.  `stats` (a dict) counts, over voxels and frames,
  which way each step went."""
  assert tsdf.dtype == F32 and weight.dtype == F32 and (color is None) == (rgb is None)
  proj, depth = np.asarray(proj, F32), np.asarray(depth, F32)
  acc = None if acc is None else np.asarray(acc, F32)
  rgb = None if rgb is None else np.asarray(rgb, F32)
  for f0 in range(0, depth.shape[0], MAX_FRAMES):
    sl = slice(f0, f0 + MAX_FRAMES)
    _integrate_launch(tsdf, weight, color, origin, spacing, trunc, proj[sl], depth[sl], None if acc is None else acc[sl],
                      None if rgb is None else rgb[sl], acc_threshold, stats)


def _integrate_launch(tsdf, weight, color, origin, spacing, trunc, proj, depth, acc, rgb, acc_threshold, stats):
  nx, ny, nz = tsdf.shape
  F, H, W = depth.shape
  spacing, trunc, thr = F32(spacing), F32(trunc), F32(acc_threshold)
  origin = np.asarray(origin, F32)
  i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
  x, y, z = (origin[d] + spacing * idx.astype(F32) for d, idx in enumerate((i, j, k)))               # step 1
  sum_t, sum_w = np.zeros(tsdf.shape, F32), np.zeros(tsdf.shape, F32)
  sum_c = np.zeros(tsdf.shape + (3,), F32)
  count = lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(m.sum())) if stats is not None else None
  with np.errstate(all='ignore'):
    for f in range(F):
      P = proj[f]
      m = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]                   # step 2
      zc = m[2]
      front = zc > 0
      u, v = m[0] / zc, m[1] / zc                                                                    # step 3
      ok = front & (u >= 0) & (u < F32(W)) & (v >= 0) & (v < F32(H))
      px, py = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
      empty = ok & (acc[f, py, px] < thr) if acc is not None else np.zeros(ok.shape, bool)           # step 4
      d = depth[f, py, px]                                                                           # step 5
      measured = ok & ~empty & (d > 0) & (d < np.inf)
      s = d - zc
      occluded = measured & (s < -trunc)
      surface = measured & ~occluded
      t = np.where(empty, F32(1), np.minimum(F32(1), s / trunc)).astype(F32)
      add = empty | surface
      sum_t[add] = sum_t[add] + t[add]                                                               # step 6
      sum_w[add] = sum_w[add] + F32(1)
      if rgb is not None:
        sum_c[add] = sum_c[add] + rgb[f, py, px][add]
      count('behind', ~front)
      count('off_image', front & ~ok)
      count('empty', empty)
      count('no_measurement', ok & ~empty & ~measured)
      count('occluded', occluded)
      count('near', surface & (s < trunc))
      count('far', surface & ~(s < trunc))
    seen = sum_w > 0                                                                                 # step 7
    W0 = weight[seen]
    Wn = W0 + sum_w[seen]
    tsdf[seen] = (W0 * tsdf[seen] + sum_t[seen]) / Wn
    if color is not None:
      color[seen] = (W0[:, None] * color[seen] + sum_c[seen]) / Wn[:, None]
    weight[seen] = Wn
  assert tsdf.dtype == F32 and weight.dtype == F32


def new_volume(shape, colors=True):
  """(tsdf, weight, color) as TsdfVolume starts them."""
  return np.ones(shape, F32), np.zeros(shape, F32), (np.zeros(tuple(shape) + (3,), F32) if colors else None)


# ---- the validity filter


def edge_keys(field, level):
  """Rows (i, j, k, e) of the grid edges that carry a vertex, lexicographic: the vertex order of csrc/mesh.hip."""
  f = np.asarray(field, F32)
  nx, ny, nz = f.shape
  with np.errstate(invalid='ignore'):
    inside = f >= F32(level)
  carries = np.zeros((nx, ny, nz, 7), bool)
  for e, (dx, dy, dz) in enumerate(R.DIRS):
    carries[:nx - dx, :ny - dy, :nz - dz, e] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
  return np.argwhere(carries)


def filter_mesh(field, level, valid, verts, normals, faces):
  """The mesh of R.marching_tetrahedra(field, level, ...) restricted to valid points -> (verts, normals, faces, keys): a vertex
  is kept iff both ends of its edge are valid, a face iff its three vertices are, unreferenced vertices go, faces are
  re-indexed; `keys` are the surviving vertices' (i, j, k, e)."""
  valid = np.asarray(valid).astype(bool)
  keys = edge_keys(field, level)
  assert len(keys) == len(verts)
  lower = keys[:, :3]
  upper = lower + np.array(R.DIRS)[keys[:, 3]]
  keep_v = valid[tuple(lower.T)] & valid[tuple(upper.T)]
  faces = faces[keep_v[faces].all(-1)] if len(faces) else faces
  used = np.zeros(len(verts), bool)
  used[faces.reshape(-1)] = True
  new_id = np.cumsum(used) - 1
  return verts[used], normals[used], new_id[faces].astype(np.int32).reshape(-1, 3), keys[used]


def volume_mesh(tsdf, weight, color, origin, spacing):
  """TsdfVolume.mesh -> dict(vertices, normals, faces, colors, faces_unfiltered)."""
  valid = weight > 0
  field = np.where(valid, -tsdf, F32(-1)).astype(F32)
  v, n, f = R.marching_tetrahedra(field, 0., origin, spacing)
  verts, normals, faces, keys = filter_mesh(field, 0., valid, v, n, f)
  cols = None
  if color is not None:
    lower = keys[:, :3]
    upper = lower + np.array(R.DIRS)[keys[:, 3]]
    f0, f1 = field[tuple(lower.T)], field[tuple(upper.T)]
    with np.errstate(all='ignore'):
      t = (F32(0) - f0) / (f1 - f0)
      t = np.where((t >= 0) & (t <= 1), t, F32(0.5)).astype(F32)[:, None]
    c0, c1 = color[tuple(lower.T)], color[tuple(upper.T)]
    c = c0 + t * (c1 - c0)
    assert c.dtype == F32
    cols = np.floor(np.clip(c, F32(0), F32(1)) * F32(255) + F32(0.5)).astype(np.uint8)
  return dict(vertices=verts, normals=normals, faces=faces, colors=cols, faces_unfiltered=len(f))


# ---- cameras and the analytic sphere scene


def look_at(position, target=(0., 0., 0.)):
  """[3,4] float64 camera-to-world (OpenGL: columns right, up, -forward, position) of a camera at `position` looking at
  `target`, up (0,0,1), or (0,1,0) where |forward.z| >= 0.9."""
  c = np.asarray(position, np.float64)
  fwd = np.asarray(target, np.float64) - c
  fwd /= np.linalg.norm(fwd)
  up0 = np.array([0., 1., 0.]) if abs(fwd[2]) >= 0.9 else np.array([0., 0., 1.])
  right = np.cross(fwd, up0)
  right /= np.linalg.norm(right)
  return np.stack([right, np.cross(right, fwd), -fwd, c], -1)


def intrinsics(fx, fy, cx, cy):
  return np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])


def projection(K, c2w):
  """[3,4] float32: K diag(1,-1,-1) [R^T | -R^T o], in float64."""
  Rm, o = c2w[:, :3], c2w[:, 3]
  return (K @ np.diag([1., -1., -1.]) @ np.concatenate([Rm.T, -(Rm.T @ o)[:, None]], 1)).astype(F32)


SPHERE_RADIUS, SPHERE_BOX, SPHERE_RES, SPHERE_TRUNC_VOXELS = 0.6, ((-1., -1., -1.), (1., 1., 1.)), 33, 3.0
SPHERE_SPACING = 2. / 32


def sphere_cameras():
  """12 positions: two rings of 5 at distance 2.5 with z / 2.5 = -0.5 and +0.5, the upper ring turned by half a step, and two
  near the poles."""
  pos = []
  for zrel, turn in ((-0.5, 0.), (0.5, 0.5)):
    for n in range(5):
      phi = 2. * math.pi * (n + turn) / 5.
      rho = math.sqrt(1. - zrel * zrel)
      pos.append((2.5 * rho * math.cos(phi), 2.5 * rho * math.sin(phi), 2.5 * zrel))
  return pos + [(0.01, 0., 2.5), (0., 0.01, -2.5)]


def render_sphere(c2w, K, H, W, radius=SPHERE_RADIUS):
  """(depth [H,W], acc [H,W], rgb [H,W,3]) float32 of the sphere |x| = radius seen through the pixel centres: the z-depth of the
  hit (0 on a miss), 1 / 0, and 0.5 + 0.5 normal (1 on a miss)."""
  ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
  cam = np.stack([xs + .5, ys + .5, np.ones_like(xs, dtype=np.float64)], -1) @ np.linalg.inv(K).T * np.array([1., -1., -1.])
  d = cam @ c2w[:, :3].T                                    # camera-space z = -1: the ray parameter IS the z-depth
  o = c2w[:, 3]
  a, b, c = (d * d).sum(-1), (d @ o), o @ o - radius * radius
  disc = b * b - a * c
  hit = disc > 0
  t = (-b - np.sqrt(np.maximum(disc, 0.))) / a
  hit &= t > 0
  n = (o + d * t[..., None]) / radius
  return (np.where(hit, t, 0.).astype(F32), hit.astype(F32), np.where(hit[..., None], 0.5 + 0.5 * n, 1.).astype(F32))


@functools.lru_cache(maxsize=None)
def sphere_scene():
  """dict(proj [12,3,4], depth [12,96,96], acc, rgb [12,96,96,3]) of the sphere scene, read-only."""
  K = intrinsics(96., 96., 48., 48.)
  cams = [look_at(p) for p in sphere_cameras()]
  frames = [render_sphere(c, K, 96, 96) for c in cams]
  out = dict(proj=np.stack([projection(K, c) for c in cams]), depth=np.stack([f[0] for f in frames]),
             acc=np.stack([f[1] for f in frames]), rgb=np.stack([f[2] for f in frames]))
  for a in out.values():
    a.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def sphere_reference():
  """The restatement alone on the sphere scene: dict(tsdf, weight, color, mesh), read-only."""
  s = sphere_scene()
  tsdf, weight, color = new_volume((SPHERE_RES,) * 3)
  integrate(tsdf, weight, color, SPHERE_BOX[0], SPHERE_SPACING, F32(SPHERE_TRUNC_VOXELS * SPHERE_SPACING), s['proj'], s['depth'],
            acc=s['acc'], rgb=s['rgb'])
  m = volume_mesh(tsdf, weight, color, SPHERE_BOX[0], SPHERE_SPACING)
  for a in (tsdf, weight, color) + tuple(v for v in m.values() if isinstance(v, np.ndarray)):
    a.setflags(write=False)
  return dict(tsdf=tsdf, weight=weight, color=color, mesh=m)


def check_sphere_mesh(verts, normals, faces, stats):
  """The conditions a fused mesh of the sphere scene meets; returns the figures."""
  r = np.linalg.norm(np.asarray(verts, np.float64), axis=1)
  dev = float(np.abs(r - SPHERE_RADIUS).max())
  ratio = stats['signed_volume'] / (4. / 3. * math.pi * SPHERE_RADIUS ** 3)
  radial = (np.asarray(normals, np.float64) * (np.asarray(verts, np.float64) / r[:, None])).sum(-1).min()
  print(f'sphere scene: V {stats["V"]} T {stats["T"]}, max |r - {SPHERE_RADIUS}| {dev:.4f}, volume ratio {ratio:.4f}, '
        f'min normal.radial {radial:.3f}')
  assert stats['euler'] == 2 and stats['boundary_edges'] == 0 and stats['nonmanifold_edges'] == 0
  assert R.directed_edges_once(faces) and stats['signed_volume'] > 0
  assert dev <= SPHERE_SPACING                              # every vertex within one grid spacing of the sphere
  assert radial > 0.8
  return dict(max_dev=dev, volume_ratio=ratio, min_normal_dot_radial=float(radial))
