"""NumPy restatement of the forward camera model (csrc/camera_project.h; include/mnerf.h, "The forward camera model"), vectorised
over points: `project` once in float64 and once in float32 in the kernel's operation order (for the perspective model, which
uses only + - x / and comparisons, the float32 one reproduces the kernel bit for bit), and `integrate`, the general-camera fusion
of mnr_tsdf_integrate_cam: tests/tsdf_ref.py's seven steps with steps 2 and 3 replaced by `project` and zc by s.

What is NOT restated: the brick mapping and the per-brick culling.  Every frame is looked at for every voxel here, so agreement
with the kernel is also the proof that its culling changes nothing.

Also here: the spherical camera's directions restated from mnr_spherical_rays' header, and the cameras the tests share.
"""

import math

import numpy as np

from tests import tsdf_ref as T

F32, F64 = np.float32, np.float64
REC = 28                                                    # MNR_CAM_REC
PERSPECTIVE, FISHEYE, PANO = 0, 1, 2                        # mnr_camtype
MAX_FRAMES = T.MAX_FRAMES


def project(rec, points, dtype=F64):
  """dict(u, v, s, ok, lhs) of points [..,3] through the record `rec` [28] (the float32 values the kernel reads), computed in `dtype`.
  ok: in front of the model and inside the fold-back guard; lhs: the guard's left side (X X + Y Y, for fisheye theta theta; 0 for
  pano), to be compared with rec[24].  dtype = float32 follows the kernel's order operation by operation."""
  rec = np.asarray(rec, F32).astype(dtype)
  p = np.asarray(points).astype(dtype)
  x, y, z = p[..., 0], p[..., 1], p[..., 2]
  model, Hf, Wf = int(rec[25]), rec[26], rec[27]
  one, two, half = dtype(1), dtype(2), dtype(0.5)
  with np.errstate(all='ignore'):
    c = [((rec[4 * r] * x + rec[4 * r + 1] * y) + rec[4 * r + 2] * z) + rec[4 * r + 3] for r in range(3)]
    if model == PANO:
      two_pi, pi = (dtype(F32(6.2831855)), dtype(F32(3.1415927))) if dtype is F32 else (dtype(2. * math.pi), dtype(math.pi))
      s = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
      ny = np.minimum(one, np.maximum(-one, -c[1] / s))
      phi = np.arccos(ny)
      theta = np.arctan2(-c[0], -c[2])
      theta = np.where(theta < 0, theta + two_pi, theta)
      u = theta * Wf / two_pi + half
      u = np.where(u >= Wf, u - Wf, u)
      v = phi * Hf / pi + half
      v = np.where(v >= Hf, Hf - half, v)
      ok = (s > 0) & (s < np.inf)
      out = dict(u=u, v=v, s=s, ok=ok, lhs=np.zeros_like(s))
    else:
      if model == FISHEYE:
        h2 = c[0] * c[0] + c[1] * c[1]
        h = np.sqrt(h2)
        theta = np.arctan2(h, c[2])
        q = np.where(h > 0, theta / np.where(h > 0, h, one), dtype(0))
        X, Y = q * c[0], q * c[1]
        s = np.sqrt(h2 + c[2] * c[2])
        lhs = theta * theta
        ok = (lhs <= rec[24]) & ((h > 0) | (c[2] > 0))
        r = X * X + Y * Y
      else:
        X, Y, s = c[0] / c[2], c[1] / c[2], c[2]
        r = X * X + Y * Y
        lhs = r
        ok = (c[2] > 0) & (r <= rec[24])
      k1, k2, k3, k4, p1, p2 = rec[18:24]
      d = one + r * (k1 + r * (k2 + r * (k3 + r * k4)))
      xd = d * X + two * p1 * X * Y + p2 * (r + two * X * X)
      yd = d * Y + two * p2 * X * Y + p1 * (r + two * Y * Y)
      u = (rec[12] * xd + rec[13] * yd) + rec[14]
      v = (rec[15] * xd + rec[16] * yd) + rec[17]
      out = dict(u=u, v=v, s=s, ok=ok, lhs=lhs)
  assert all(a.dtype == (bool if n == 'ok' else dtype) for n, a in out.items())
  return out


def on_image(pr, rec):
  """The kernel's `valid`: ok and 0 <= u < W and 0 <= v < H."""
  Hf, Wf = pr['u'].dtype.type(rec[26]), pr['u'].dtype.type(rec[27])
  with np.errstate(invalid='ignore'):
    return pr['ok'] & (pr['u'] >= 0) & (pr['u'] < Wf) & (pr['v'] >= 0) & (pr['v'] < Hf)


def deviation(rec, points):
  """The float32 restatement's worst deviation from the float64 one over the points that float64 puts on the image:
  dict(uv, s, lhs) in pixels, world units and the guard's units.  A pano column near the seam may differ by the whole width W in u
  while naming the same direction, so |du| is taken modulo W there."""
  a, b = project(rec, points, F64), project(rec, points, F32)
  m = on_image(a, rec)
  if not m.any():
    return dict(uv=0., s=0., lhs=0.)
  du = np.abs(a['u'] - b['u'].astype(F64))[m]
  if int(rec[25]) == PANO:
    du = np.minimum(du, np.abs(float(rec[27]) - du))
  dv = np.abs(a['v'] - b['v'].astype(F64))[m]
  return dict(uv=float(max(du.max(), dv.max())), s=float(np.abs(a['s'] - b['s'].astype(F64))[m].max()),
              lhs=float(np.abs(a['lhs'] - b['lhs'].astype(F64))[m].max()))


def undecided(pr, rec, delta):
  """True where the float64 projection `pr` is within delta['uv'] of a pixel edge (edges are the integers, the image's border
  included) or within delta['lhs'] of the guard: a float32 evaluation may take the other side there."""
  near = lambda a: np.abs(a - np.round(a)) < delta['uv']
  with np.errstate(invalid='ignore'):
    out = near(pr['u']) | near(pr['v'])
    if int(rec[25]) != PANO:
      out |= np.abs(pr['lhs'] - F64(F32(rec[24]))) < delta['lhs']
  return out


def integrate(tsdf, weight, color, origin, spacing, trunc, cameras, depth, acc=None, rgb=None, acc_threshold=0.5, stats=None, dtype=F32,
              delta=None):
  """mnr_tsdf_integrate_cam: updates tsdf, weight [nx,ny,nz] and color (or None) in place; the volumes are of `dtype`.

  dtype = float32 is the kernel's arithmetic in its order (bit for bit for the perspective model).  dtype = float64 is the
  reference for fisheye and pano: the voxel coordinates are still the kernel's float32 ones, everything after them is float64.
  `stats` counts the branches as tests/tsdf_ref.py does, plus `guarded`: in front of the camera but outside the fold-back guard.
  With `delta` (dict(uv, s, lhs), see `undecided`) it returns (decided [nx,ny,nz] bool: every (voxel, frame) pair of the voxel is
  decided, the number of undecided pairs, the number of pairs on the image)."""
  assert tsdf.dtype == dtype and weight.dtype == dtype and (color is None) == (rgb is None)
  cameras, depth = np.asarray(cameras, F32), np.asarray(depth, F32)
  acc = None if acc is None else np.asarray(acc, F32)
  rgb = None if rgb is None else np.asarray(rgb, F32)
  decided, n_undecided, n_pairs = np.ones(tsdf.shape, bool), 0, 0
  for f0 in range(0, depth.shape[0], MAX_FRAMES):
    sl = slice(f0, f0 + MAX_FRAMES)
    d, nu, npair = _launch(tsdf, weight, color, origin, spacing, trunc, cameras[sl], depth[sl], None if acc is None else acc[sl],
                           None if rgb is None else rgb[sl], acc_threshold, stats, dtype, delta)
    decided &= d
    n_undecided += nu
    n_pairs += npair
  return (decided, n_undecided, n_pairs) if delta is not None else None


def _launch(tsdf, weight, color, origin, spacing, trunc, cameras, depth, acc, rgb, acc_threshold, stats, dtype, delta):
  nx, ny, nz = tsdf.shape
  F, H, W = depth.shape
  trunc, thr = dtype(F32(trunc)), F32(acc_threshold)
  origin = np.asarray(origin, F32)
  i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
  xyz = np.stack([origin[d] + F32(spacing) * idx.astype(F32) for d, idx in enumerate((i, j, k))], -1)   # step 1, float32 always
  assert xyz.dtype == F32
  sum_t, sum_w = np.zeros(tsdf.shape, dtype), np.zeros(tsdf.shape, dtype)
  sum_c = np.zeros(tsdf.shape + (3,), dtype)
  count = lambda name, m: stats.__setitem__(name, stats.get(name, 0) + int(m.sum())) if stats is not None else None
  decided, n_undecided, n_pairs = np.ones(tsdf.shape, bool), 0, 0
  with np.errstate(all='ignore'):
    for f in range(F):
      rec = cameras[f]
      pr = project(rec, xyz, dtype)                                                                  # steps 2 and 3
      ok = on_image(pr, rec)
      s = pr['s']
      px, py = np.where(ok, pr['u'], 0).astype(np.int64), np.where(ok, pr['v'], 0).astype(np.int64)
      empty = ok & (acc[f, py, px] < thr) if acc is not None else np.zeros(ok.shape, bool)           # step 4
      d = depth[f, py, px].astype(dtype)                                                             # step 5
      measured = ok & ~empty & (d > 0) & (d < np.inf)
      e = d - s
      occluded = measured & (e < -trunc)
      surface = measured & ~occluded
      t = np.where(empty, dtype(1), np.minimum(dtype(1), e / trunc)).astype(dtype)
      add = empty | surface
      sum_t[add] = sum_t[add] + t[add]                                                               # step 6
      sum_w[add] = sum_w[add] + dtype(1)
      if rgb is not None:
        sum_c[add] = sum_c[add] + rgb[f, py, px][add].astype(dtype)
      if int(rec[25]) == PERSPECTIVE:
        front = s > 0
      else:
        front = pr['ok'] | (pr['lhs'] > rec[24].astype(dtype))
      count('behind', ~front)
      count('guarded', front & ~pr['ok'])
      count('off_image', pr['ok'] & ~ok)
      count('empty', empty)
      count('no_measurement', ok & ~empty & ~measured)
      count('occluded', occluded)
      count('near', surface & (e < trunc))
      count('far', surface & ~(e < trunc))
      if delta is not None:
        # a pair matters if the point is on the image, or so close to its border or to the guard that float32 may put it there
        und = undecided(pr, rec, delta)
        inside = np.abs(np.clip(pr['u'], 0., float(W)) - pr['u']) < delta['uv']
        inside &= np.abs(np.clip(pr['v'], 0., float(H)) - pr['v']) < delta['uv']
        if int(rec[25]) != PANO:
          inside &= pr['lhs'] < F64(rec[24]) + delta['lhs']
          inside &= front
        und = und & inside
        und |= measured & ((np.abs(e + trunc) < delta['s']) | (np.abs(e - trunc) < delta['s']))
        decided &= ~und
        n_undecided += int(und.sum())
        n_pairs += int(ok.sum())
    seen = sum_w > 0                                                                                 # step 7
    W0 = weight[seen]
    Wn = W0 + sum_w[seen]
    tsdf[seen] = (W0 * tsdf[seen] + sum_t[seen]) / Wn
    if color is not None:
      color[seen] = (W0[:, None] * color[seen] + sum_c[seen]) / Wn[:, None]
    weight[seen] = Wn
  assert tsdf.dtype == dtype and weight.dtype == dtype
  return decided, n_undecided, n_pairs


def new_volume(shape, colors=True, dtype=F32):
  return np.ones(shape, dtype), np.zeros(shape, dtype), (np.zeros(tuple(shape) + (3,), dtype) if colors else None)


# ---- the project's own rays, restated


def spherical_directions(c2w, H, W):
  """directions [H,W,3] float64 of mnr_spherical_rays (its header): pixel (h, w) looks along R (-sin phi sin theta, cos phi,
  sin phi cos theta) at theta = 2 pi w / W, phi = pi h / H."""
  theta = (np.arange(W) * (2. * math.pi / W))[None, :]
  phi = (np.arange(H) * (math.pi / H))[:, None]
  c = np.stack([-np.sin(phi) * np.sin(theta), np.cos(phi) * np.ones_like(theta), np.sin(phi) * np.cos(theta)], -1)
  return c @ np.asarray(c2w, F64)[:, :3].T


# ---- cameras the tests share

H, W = 24, 20
DISTORTION = dict(k1=-0.05, k2=0.004, p1=0.002, p2=-0.003)   # mild: the 24 x 20 images below stay inside the invertible region
FISHEYE_DISTORTION = dict(k1=0.02, k2=-0.003, p1=0.001, p2=-0.0015)


def poses():
  """[3] camera-to-world matrices like tests/test_gpu_tsdf.cameras(): one that sees the whole grid from outside, one INSIDE the
  box, one that sees about half of the box."""
  return [T.look_at((2.1, 1.7, 1.3)), T.look_at((0.01, 0.02, 0.3), target=(0.3, -0.2, 1.)), T.look_at((3., 0.2, 0.1), target=(0., 0., 1.6))]


def intrinsics():
  """[3] K matrices for `poses`: fx != fy and an off-centre principal point first."""
  K = T.intrinsics(15., 15., W / 2., H / 2.)
  return [T.intrinsics(13., 17., 8.7, 13.1), K, K]


def fisheye_intrinsics():
  """Fisheye cameras see wide: 7 pixels a radian put the 24 x 20 image's corners at theta = 2.2."""
  K = T.intrinsics(7., 7., W / 2., H / 2.)
  return [T.intrinsics(6.5, 7.5, 9.3, 12.6), K, K]


def record(K, c2w, camtype='perspective', distortion=None, height=H, width=W):
  """mesh.camera_record for an intrinsics matrix K (None for a pano)."""
  from multinerf_amd import mesh
  return mesh.camera_record(None if K is None else np.linalg.inv(K), c2w, height, width, distortion_params=distortion, camtype=camtype)


# ---- the analytic scenes: depth is the Euclidean distance along unit rays

FISHEYE_SPHERE_IMAGE = 96        # 96 x 96 pixels at 96 pixels a radian: the pinhole scene's sampling on the optical axis
INSIDE_RADIUS, PANO_IMAGE = 0.8, (64, 128)
PANO_EYES = ((0.05, 0.02, -0.03), (-0.04, 0.03, 0.06))


def _render_ball(origin, d, radius, inside):
  """(depth, acc, rgb) of the sphere |x| = radius along unit rays origin + t d [..,3]: the near hit from outside (0 / 0 / white on a
  miss), the far one from inside; rgb = 0.5 + 0.5 outward normal."""
  b, c = d @ origin, origin @ origin - radius * radius
  disc = b * b - c
  root = np.sqrt(np.maximum(disc, 0.))
  t = -b + root if inside else -b - root
  hit = (disc > 0) & (t > 0)
  n = (origin + d * t[..., None]) / radius
  return np.where(hit, t, 0.).astype(F32), hit.astype(F32), np.where(hit[..., None], 0.5 + 0.5 * n, 1.).astype(F32)


def fisheye_directions(K, c2w, height, width):
  """Unit directions [H,W,3] float64 of an undistorted fisheye camera's pixel centres (camera.hip's ray model)."""
  ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing='ij')
  p = np.stack([xs + .5, ys + .5, np.ones_like(xs, dtype=F64)], -1) @ np.linalg.inv(K).T
  theta = np.minimum(np.hypot(p[..., 0], p[..., 1]), math.pi)
  sot = np.sin(theta) / theta
  cam = np.stack([p[..., 0] * sot, -p[..., 1] * sot, -np.cos(theta)], -1)                            # OpenCV -> OpenGL
  return cam @ np.asarray(c2w, F64)[:, :3].T


def fisheye_sphere_scene():
  """The sphere of tests/tsdf_ref.py seen by its 12 positions as fisheye cameras: dict(cameras [12,28], depth, acc [12,96,96], rgb)."""
  n = FISHEYE_SPHERE_IMAGE
  K = T.intrinsics(float(n), float(n), n / 2., n / 2.)
  poses_ = [T.look_at(p) for p in T.sphere_cameras()]
  frames = [_render_ball(c[:, 3], fisheye_directions(K, c, n, n), T.SPHERE_RADIUS, False) for c in poses_]
  return dict(cameras=np.stack([record(K, c, 'fisheye', height=n, width=n) for c in poses_]), depth=np.stack([f[0] for f in frames]),
              acc=np.stack([f[1] for f in frames]), rgb=np.stack([f[2] for f in frames]))


def inside_out_scene():
  """The inside of the sphere |x| = 0.8 seen by two pano cameras near its centre: dict(cameras [2,28], depth, acc [2,64,128], rgb)."""
  Hp, Wp = PANO_IMAGE
  poses_ = [np.concatenate([np.eye(3), np.array(e)[:, None]], 1) for e in PANO_EYES]
  poses_[1][:, :3] = T.look_at((1., 2., 0.5))[:, :3]                                                 # (the second one turned)
  frames = [_render_ball(c[:, 3], spherical_directions(c, Hp, Wp), INSIDE_RADIUS, True) for c in poses_]
  return dict(cameras=np.stack([record(None, c, 'pano', height=Hp, width=Wp) for c in poses_]), depth=np.stack([f[0] for f in frames]),
              acc=np.stack([f[1] for f in frames]), rgb=np.stack([f[2] for f in frames]))


def check_inside_out_mesh(verts, normals, faces, stats):
  """tests/tsdf_ref.check_sphere_mesh's conditions for the sphere seen from INSIDE: free space is the inside, so the faces are
  counter-clockwise seen from there, the signed volume is negative and the normals point to the centre."""
  from tests import mesh_ref as R
  r = np.linalg.norm(np.asarray(verts, F64), axis=1)
  dev = float(np.abs(r - INSIDE_RADIUS).max())
  ratio = stats['signed_volume'] / (4. / 3. * math.pi * INSIDE_RADIUS ** 3)
  radial = (np.asarray(normals, F64) * (np.asarray(verts, F64) / r[:, None])).sum(-1).max()
  print(f'inside-out scene: V {stats["V"]} T {stats["T"]}, max |r - {INSIDE_RADIUS}| {dev:.4f}, volume ratio {ratio:.4f}, '
        f'max normal.radial {radial:.3f}')
  assert stats['euler'] == 2 and stats['boundary_edges'] == 0 and stats['nonmanifold_edges'] == 0
  assert R.directed_edges_once(faces) and stats['signed_volume'] < 0
  assert dev <= T.SPHERE_SPACING                            # every vertex within one grid spacing of the sphere
  assert radial < -0.8
  return dict(max_dev=dev, volume_ratio=ratio, max_normal_dot_radial=float(radial))
