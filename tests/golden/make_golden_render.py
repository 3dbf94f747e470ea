#!/usr/bin/env python
"""Record the reference's own camera paths, spherical camera and visualisations (internal/camera_utils.py, internal/vis.py).

    python tests/golden/make_golden_render.py            # writes tests/golden/render_path.npz

The reference modules are imported FROM WHERE THEY LIE (MULTINERF_REFERENCE, nothing is copied) on the NumPy stand-in of
tests/golden/make_golden.py (float64), with the internal.configs / internal.utils stubs of make_golden_pca.py (utils.Rays
becomes a plain record).  Two stand-ins beyond those:

  * a clamped gather for `w[sortidx]` in vis.weighted_percentile.  jax documents that an out-of-range index of x[indices]
    is clamped; visualize_suite relies on it for the depth triplet (value [H,W,3] and weight [H,W], both flattened); NumPy
    raises instead.  The function is wrapped: the wrapper orders the data (stable argsort, the weight of sorted element i
    is w[min(order[i], len(w) - 1)]) and hands it to the reference's function with assume_sorted=True, so the cumulative
    sum and the interpolation that are recorded are the reference's own lines.  jax cannot be run here, so the clamp
    rests on its documentation.
  * `matplotlib.cm.get_cmap`, which newer matplotlib releases no longer have, mapped to `matplotlib.colormaps[name]`.

The .npz holds arrays only: inputs (float32-representable), the reference's outputs in float64, and the turbo and gray
tables the colour maps were sampled from.  The two ray panels of visualize_suite are 1983 x 2048 images in which every
(ray, level) row is repeated 41 times; the file keeps one row of each, one background strip row, and every 16th column
(`suite/panel_rows`, `suite/panel_col_step`).  Weights in the percentile cases are exactly 0 or >= 1e-3; in the case with
ties, multiples of 1/1024, so that every partial sum is exact whatever its order.
"""

import dataclasses
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as G  # noqa: E402

OUT = os.path.join(HERE, 'render_path.npz')


def f32r(x):
  """float32-representable float64."""
  return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ring_poses(rs, n, tilt=0.3):
  """n cameras on a noisy ring around the origin looking roughly at it (OpenGL axes: x right, y up, z back)."""
  ang = np.sort(rs.uniform(0, 2 * np.pi, n))
  pos = np.stack([rs.uniform(2.5, 3.5, n) * np.cos(ang), rs.uniform(2.0, 3.0, n) * np.sin(ang), tilt * rs.normal(size=n) + 0.5], 1)
  poses = []
  for p in pos:
    z = p + 0.2 * rs.normal(size=3)
    z /= np.linalg.norm(z)
    x = np.cross([0., 0., 1.], z)
    x /= np.linalg.norm(x)
    poses.append(np.stack([x, np.cross(z, x), z, p], 1))
  return np.stack(poses, 0)


def forward_poses(rs, n):
  """n cameras on a slab around the origin looking down -z, slightly turned (a recentred forward-facing capture)."""
  poses = []
  for _ in range(n):
    q, _ = np.linalg.qr(np.eye(3) + 0.08 * rs.normal(size=(3, 3)))
    q = q * np.sign(np.diag(q))
    poses.append(np.concatenate([q, (rs.normal(size=3) * [0.6, 0.4, 0.05])[:, None]], 1))
  return np.stack(poses, 0)


def install():
  jax = G.install_jax_standin()
  sys.path.insert(0, G.REF)
  cfg_stub = types.ModuleType('internal.configs')
  utils_stub = types.ModuleType('internal.utils')

  @dataclasses.dataclass
  class Rays:
    origins: object
    directions: object
    viewdirs: object
    radii: object
    imageplane: object
    lossmult: object = None
    near: object = None
    far: object = None
    cam_idx: object = None

  utils_stub.Pixels = utils_stub.Rays = Rays
  cfg_stub.Config = object
  sys.modules['internal.configs'] = cfg_stub
  sys.modules['internal.utils'] = utils_stub
  import matplotlib
  from matplotlib import cm
  if not hasattr(cm, 'get_cmap'):
    cm.get_cmap = lambda name: matplotlib.colormaps[name]
  from internal import camera_utils, vis
  ref_wp = vis.weighted_percentile

  def weighted_percentile(x, w, ps, assume_sorted=False):
    x, w = x.reshape([-1]), w.reshape([-1])
    if not assume_sorted:
      order = np.argsort(x, kind='stable')
      x, w = x[order], w[np.minimum(order, len(w) - 1)]
    return ref_wp(x, w, ps, assume_sorted=True)

  vis.weighted_percentile = weighted_percentile
  return jax, camera_utils, vis, matplotlib


def main():
  jax, camera_utils, vis, matplotlib = install()
  jnp = jax.numpy
  g = {}
  rs = np.random.RandomState(20241017)

  # ----------------------------------------------------------------------------- camera paths
  poses, bounds = forward_poses(rs, 9), rs.uniform(1.0, 10.0, (9, 2))
  g['spiral/poses'], g['spiral/bounds'] = poses, bounds
  g['spiral/out'] = camera_utils.generate_spiral_path(poses, bounds, n_frames=7)
  g['spiral/out_rots'] = camera_utils.generate_spiral_path(poses, bounds, n_frames=7, n_rots=1, zrate=0.25)
  poses = ring_poses(rs, 11)
  g['ellipse/poses'] = poses
  g['ellipse/out_const'] = camera_utils.generate_ellipse_path(poses, n_frames=8, const_speed=True, z_variation=0.3, z_phase=0.25)
  g['ellipse/out_plain'] = camera_utils.generate_ellipse_path(poses, n_frames=8, const_speed=False, z_variation=0.3, z_phase=0.25)
  g['ellipse/out_flat'] = camera_utils.generate_ellipse_path(poses, n_frames=8)
  keys = ring_poses(rs, 4)
  g['interp/poses'] = keys
  g['interp/out'] = camera_utils.generate_interpolated_path(keys, n_interp=5, spline_degree=5, smoothness=.03, rot_weight=.1)
  keys7 = ring_poses(rs, 7)
  g['interp/poses7'] = keys7
  g['interp/out7'] = camera_utils.generate_interpolated_path(keys7, n_interp=3, spline_degree=5, smoothness=.03, rot_weight=.1)
  x = np.log(rs.uniform(0.5, 4.0, 9))
  g['interp1d/x'] = x
  g['interp1d/out'] = np.asarray(camera_utils.interpolate_1d(x, 4, spline_degree=5, smoothness=20))
  g['interp1d/out_k3'] = np.asarray(camera_utils.interpolate_1d(x, 3, spline_degree=3, smoothness=0.05))

  # ----------------------------------------------------------------------------- spherical camera
  for H, W in ((6, 9), (17, 32)):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    c2w = f32r(np.concatenate([q, rs.normal(size=(3, 1)) * 2], 1))
    rays = camera_utils.cast_spherical_rays(c2w, H, W, 0.2, 1e6, xnp=np)
    tag = f'sph_{H}x{W}'
    g[f'{tag}/c2w'] = c2w
    g[f'{tag}/origins'], g[f'{tag}/directions'], g[f'{tag}/viewdirs'] = rays.origins.copy(), rays.directions, rays.viewdirs
    g[f'{tag}/radii'], g[f'{tag}/imageplane'] = rays.radii, rays.imageplane
    assert rays.lossmult.shape == (H, W, 1) and float(rays.near[0, 0, 0]) == 0.2 and int(rays.cam_idx[0, 0, 0]) == 0

  # ----------------------------------------------------------------------------- weighted percentile
  def weights(shape, zero_share=0.1):
    w = rs.uniform(1e-3, 1.0, shape)
    w[rs.uniform(size=shape) < zero_share] = 0.0
    w = f32r(w)
    assert ((w == 0) | (w >= 1e-3)).all()
    return w

  for tag, shape in (('wp_a', (37, 53)), ('wp_b', (3, 5))):
    x, w = f32r(rs.uniform(2, 6, shape)), weights(shape)
    g[f'{tag}/x'], g[f'{tag}/w'] = x, w
    g[f'{tag}/ps'] = np.array([0.5, 99.5, 5., 50.])
    g[f'{tag}/out'] = vis.weighted_percentile(x, w, list(g[f'{tag}/ps']))
  x, w = f32r(rs.uniform(0.5, 8, (7, 9, 3))), weights((7, 9))
  g['wp_triplet/x'], g['wp_triplet/w'], g['wp_triplet/ps'] = x, w, np.array([0.5, 99.5])
  g['wp_triplet/out'] = vis.weighted_percentile(x, w, [0.5, 99.5])
  xs = np.sort(rs.randint(0, 10, 60)).astype(np.float64)                 # ties
  ws = rs.randint(1, 1025, 60) / 1024.
  ws[:3] = 0.0                                                           # zero weights in front and at the end, and inside
  ws[-4:] = 0.0
  ws[rs.choice(np.arange(5, 50), 6, replace=False)] = 0.0
  assert ((ws == 0) | (ws >= 1e-3)).all()
  perm = rs.permutation(60)
  # (a stable sort keeps the shuffled order inside a tie; the zero weights are placed after the shuffle is undone, so they
  # sit at the two ends of the SORTED array whatever the tie order)
  order = np.argsort(xs[perm], kind='stable')
  w_shuffled = np.empty(60)
  w_shuffled[order] = ws
  g['wp_tied/x'], g['wp_tied/w'], g['wp_tied/ps'] = xs[perm], w_shuffled, np.array([0., 0.5, 50., 99.5, 100.])
  g['wp_tied/out'] = vis.weighted_percentile(xs[perm], w_shuffled, list(g['wp_tied/ps']))
  g['wp_zero/x'], g['wp_zero/w'], g['wp_zero/ps'] = f32r(rs.uniform(0, 1, 70)), np.zeros(70), np.array([0., 50., 100.])
  g['wp_zero/out'] = vis.weighted_percentile(g['wp_zero/x'], g['wp_zero/w'], [0., 50., 100.])

  # ----------------------------------------------------------------------------- visualize_cmap
  turbo, gray = matplotlib.colormaps['turbo'], matplotlib.colormaps['gray']
  g['lut/turbo'] = np.asarray(turbo(np.arange(turbo.N)), np.float64)[:, :3]
  g['lut/gray'] = np.asarray(gray(np.arange(gray.N)), np.float64)[:, :3]
  eps = float(np.finfo(np.float32).eps)
  neg_log = lambda z: -jnp.log(z + eps)
  log = lambda z: jnp.log(z + eps)
  H, W = 37, 53
  value, weight = f32r(rs.uniform(2, 6, (H, W))), weights((H, W), 0.15)
  weight = np.minimum(weight, 1.0)
  g['cmap/value'], g['cmap/weight'] = value, weight
  g['cmap/lohi'] = vis.weighted_percentile(value, weight, [0.5, 99.5])
  g['cmap/out'] = vis.visualize_cmap(value, weight, turbo, curve_fn=neg_log)
  g['cmap/out_lohi'] = vis.visualize_cmap(value, weight, turbo, lo=2.5, hi=5.0, curve_fn=neg_log, matte_background=False)
  g['cmap/out_mod'] = vis.visualize_cmap(value, weight, turbo, modulus=0.25)
  value3 = f32r(rs.uniform(0.5, 8, (H, W, 3)))
  g['cmap/value3'] = value3
  g['cmap/lohi3'] = vis.weighted_percentile(value3, weight, [0.5, 99.5])
  g['cmap/out_c3'] = vis.visualize_cmap(value3, weight, None, curve_fn=log)

  # ----------------------------------------------------------------------------- visualize_suite
  H, W, R = 24, 32, 16
  yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing='ij')
  blob = np.exp(-3 * (xx**2 + yy**2))
  acc = f32r(np.clip(1.3 * blob + 0.05 * rs.uniform(size=(H, W)), 0, 1))
  dmed = f32r(4 - 1.5 * blob + 0.05 * rs.normal(size=(H, W)))
  dmean = f32r(dmed + 0.1 * rs.normal(size=(H, W)))
  dmean[3, 5] = dmean[20, 30] = np.nan
  rendering = {
      'rgb': f32r(rs.uniform(0, 1, (H, W, 3))), 'acc': acc, 'distance_mean': dmean, 'distance_median': dmed,
      'distance_percentile_5': f32r(dmed - rs.uniform(0.01, 0.6, (H, W))),
      'distance_percentile_95': f32r(dmed + rs.uniform(0.01, 0.6, (H, W))),
      'normals': f32r(rs.normal(size=(H, W, 3)) * 0.6), 'normals_pred': f32r(rs.normal(size=(H, W, 3)) * 0.6),
      'roughness': f32r(rs.normal(size=(H, W, 1))), 'rgb_cc': f32r(rs.uniform(0, 1, (H, W, 3))),
      'ray_sdist': [], 'ray_weights': [], 'ray_rgbs': [],
  }
  for n in (8, 8, 6):
    s = np.cumsum(rs.uniform(0.05, 1.0, (R, n + 1)), -1)
    s = (s - s[:, :1]) / (s[:, -1:] - s[:, :1])
    wts = rs.dirichlet(np.ones(n + 1), R)[:, :n]
    wts[rs.uniform(size=wts.shape) < 0.15] = 0.0
    rendering['ray_sdist'].append(f32r(s))
    rendering['ray_weights'].append(f32r(wts))
    rendering['ray_rgbs'].append(f32r(rs.uniform(-0.1, 1.1, (R, n, 3))))
  rays = types.SimpleNamespace(origins=f32r(rs.normal(size=(H, W, 3))), directions=f32r(rs.normal(size=(H, W, 3)) * 0.5))
  for k, v in rendering.items():
    if isinstance(v, list):
      for lv, a in enumerate(v):
        g[f'suite/in/{k}/{lv}'] = a
    else:
      g[f'suite/in/{k}'] = v
  g['suite/in/origins'], g['suite/in/directions'] = rays.origins, rays.directions
  with np.errstate(invalid='ignore'):
    out = vis.visualize_suite(rendering, rays)
  L = 3
  rep = 2048 // (R * L + 1)
  stride = rep * L
  rows = np.array([r * (stride + 1) + lv * rep for r in range(R) for lv in range(L)] + [stride])
  g['suite/panel_rows'], g['suite/panel_col_step'] = rows, np.int64(16)
  for k, v in out.items():
    v = np.asarray(v, np.float64)
    if k in ('ray_colors', 'ray_weights'):
      assert v.shape == (R * (stride + 1) - 1, 2048, 3), v.shape
      # every row of a (ray, level) block repeats the block's first row; the strip rows are one colour
      for r in rows[:-1]:
        assert (v[r:r + rep] == v[r]).all()
      v = v[rows][:, ::16]
    g[f'suite/out/{k}'] = v
  g['suite/keys'] = np.array(sorted(out))
  np.savez_compressed(OUT, **g)
  print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(g)} arrays)')
  print('suite keys:', sorted(out))


if __name__ == '__main__':
  main()
