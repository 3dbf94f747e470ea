"""Ray generation on device: the reference's camera_utils.pixels_to_rays / cast_ray_batch
(internal/camera_utils.py:514-688) behind the same names, backed by mnr_pixels_to_rays (csrc/camera.hip).

The per-pixel leaves are device code, as are the rays of the spherical camera (mnr_spherical_rays); the
pose utilities and the render paths (spiral, ellipse, spline: camera_utils.py:159-395) run once per script on the host, in
NumPy float64.
"""

import ctypes as C
import enum

import numpy as np
import torch

from multinerf_amd import _lib as L
from multinerf_amd import ops, utils


class ProjectionType(enum.Enum):
  """camera_utils.py:514-517."""
  PERSPECTIVE = 'perspective'
  FISHEYE = 'fisheye'


_DIST_KEYS = ('k1', 'k2', 'k3', 'k4', 'p1', 'p2')


def pixels_to_rays(pix_x_int, pix_y_int, pixtocams, camtoworlds, distortion_params=None, pixtocam_ndc=None,
                   camtype=ProjectionType.PERSPECTIVE, cam_idx=None):
  """camera_utils.py:520-631.  pixtocams [3,3] or [N,3,3] (+ cam_idx [...] selecting the camera per pixel; the
  reference indexes the stacks before the call, `batch_index` camera_utils.py:665).  Device tensors in,
  (origins, directions, viewdirs, radii, imageplane) out, shaped like the pixel arrays."""
  shape = tuple(pix_x_int.shape)
  dev = pix_x_int.device
  if not ops._on_device(pix_x_int):
    raise ValueError('pixels_to_rays: device tensors required (the HIP path has no CPU fallback)')
  px = pix_x_int.reshape(-1).to(torch.int32).contiguous()
  py = pix_y_int.reshape(-1).to(torch.int32).contiguous()
  B = px.numel()
  P = pixtocams.to(device=dev, dtype=torch.float32).reshape(-1, 3, 3).contiguous()
  Cw = camtoworlds.to(device=dev, dtype=torch.float32)[..., :3, :4].reshape(-1, 3, 4).contiguous()
  ncam = max(P.shape[0], Cw.shape[0])
  if P.shape[0] != ncam:
    P = P.expand(ncam, 3, 3).contiguous()
  if Cw.shape[0] != ncam:
    Cw = Cw.expand(ncam, 3, 4).contiguous()
  ci = None
  if ncam > 1:
    if cam_idx is None:
      raise ValueError('pixels_to_rays: stacked cameras need cam_idx')
    ci = cam_idx.reshape(-1).to(torch.int32).contiguous()
  dist = None
  if distortion_params is not None:
    unknown = set(distortion_params) - set(_DIST_KEYS)
    if unknown:
      raise TypeError(f'unexpected distortion parameters {sorted(unknown)}')      # **kwargs error of the reference
    dist = (C.c_float * 6)(*[float(distortion_params.get(k, 0.0)) for k in _DIST_KEYS])
  ndc = None
  if pixtocam_ndc is not None:
    ndc = torch.as_tensor(pixtocam_ndc).to(device=dev, dtype=torch.float32).reshape(3, 3).contiguous()
  f32 = torch.float32
  origins = torch.empty((B, 3), dtype=f32, device=dev)
  directions = torch.empty((B, 3), dtype=f32, device=dev)
  viewdirs = torch.empty((B, 3), dtype=f32, device=dev)
  radii = torch.empty((B, 1), dtype=f32, device=dev)
  imageplane = torch.empty((B, 2), dtype=f32, device=dev)
  p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
  L.check(ops.lib().mnr_pixels_to_rays(
      B, p(px), p(py), p(ci), ncam, p(P), p(Cw), C.cast(dist, C.c_void_p) if dist is not None else None, p(ndc),
      1 if ProjectionType(camtype) == ProjectionType.FISHEYE else 0, p(origins), p(directions), p(viewdirs), p(radii),
      p(imageplane), ops._stream()))
  r = lambda t, c: t.reshape(shape + (c,))
  return r(origins, 3), r(directions, 3), r(viewdirs, 3), r(radii, 1), r(imageplane, 2)


def cast_ray_batch(cameras, pixels, camtype=ProjectionType.PERSPECTIVE, xnp=None):
  """camera_utils.py:634-688: utils.Pixels -> utils.Rays (`xnp` is accepted and ignored: arrays are torch)."""
  pixtocams, camtoworlds, distortion_params, pixtocam_ndc = cameras
  origins, directions, viewdirs, radii, imageplane = pixels_to_rays(
      pixels.pix_x_int, pixels.pix_y_int, pixtocams, camtoworlds, distortion_params=distortion_params,
      pixtocam_ndc=pixtocam_ndc, camtype=camtype, cam_idx=pixels.cam_idx[..., 0])
  return utils.Rays(origins=origins, directions=directions, viewdirs=viewdirs, radii=radii, imageplane=imageplane,
                    lossmult=pixels.lossmult, near=pixels.near, far=pixels.far, cam_idx=pixels.cam_idx,
                    exposure_idx=pixels.exposure_idx, exposure_values=pixels.exposure_values)


def cast_spherical_rays(camtoworld, height, width, near, far, xnp=None):
  """camera_utils.py:716-764: the rays of a spherical (panorama) camera, shaped [H, W, .] (`xnp` is accepted and ignored)."""
  origins, directions, viewdirs, radii, imageplane = ops.spherical_rays(camtoworld, height, width)
  full = lambda v, dt=torch.float32: torch.full((int(height), int(width), 1), v, dtype=dt, device=origins.device)
  return utils.Rays(origins=origins, directions=directions, viewdirs=viewdirs, radii=radii, imageplane=imageplane,
                    lossmult=full(1.), near=full(float(near)), far=full(float(far)), cam_idx=full(0, torch.int32))


def intrinsic_matrix(fx, fy, cx, cy):
  """camera_utils.py:398-408."""
  return torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], dtype=torch.float64)


def get_pixtocam(focal, width, height):
  """camera_utils.py:411-417 (inverted in fp64, returned fp32)."""
  return torch.linalg.inv(intrinsic_matrix(focal, focal, width * .5, height * .5)).float()


def pixel_coordinates(width, height, device='cpu'):
  """camera_utils.py:420-424: (x, y) integer grids, each [height, width]."""
  y, x = torch.meshgrid(torch.arange(height, device=device), torch.arange(width, device=device), indexing='ij')
  return x, y


# ----------------------------------------------------------------------------- pose utilities (host, NumPy):
# scene normalisation done once at dataset load time (camera_utils.py:101-156,191-227), not on the per-ray path.


def pad_poses(p):
  """camera_utils.py:101-104: [..., 3, 4] -> [..., 4, 4] with a [0, 0, 0, 1] bottom row."""
  bottom = np.broadcast_to([0, 0, 0, 1.], p[..., :1, :4].shape)
  return np.concatenate([p[..., :3, :4], bottom], axis=-2)


def unpad_poses(p):
  """camera_utils.py:107-109."""
  return p[..., :3, :4]


def normalize(x):
  """camera_utils.py:139-141."""
  return x / np.linalg.norm(x)


def viewmatrix(lookdir, up, position):
  """camera_utils.py:129-136."""
  vec2 = normalize(lookdir)
  vec0 = normalize(np.cross(up, vec2))
  vec1 = normalize(np.cross(vec2, vec0))
  return np.stack([vec0, vec1, vec2, position], axis=1)


def average_pose(poses):
  """camera_utils.py:120-126."""
  position = poses[:, :3, 3].mean(0)
  z_axis = poses[:, :3, 2].mean(0)
  up = poses[:, :3, 1].mean(0)
  return viewmatrix(z_axis, up, position)


def recenter_poses(poses):
  """Express all cameras in the frame of their average camera (what camera_utils.py:112-117 computes).

  Returns (poses [N,3,4], world -> average-camera transform [4,4]).  The average frame [R | c] is rigid, so its
  inverse is written down directly, [R^T | -R^T c], instead of inverting the padded 4x4.
  """
  mean_frame = average_pose(poses)
  r_t = mean_frame[:3, :3].T
  world_to_mean = np.eye(4)
  world_to_mean[:3, :3] = r_t
  world_to_mean[:3, 3] = -r_t @ mean_frame[:3, 3]
  return np.einsum('ij,njk->nik', world_to_mean[:3, :3], poses[:, :3, :4]) + \
      np.concatenate([np.zeros((3, 3)), world_to_mean[:3, 3:4]], 1)[None], world_to_mean


def focus_point_fn(poses):
  """The point closest, in the least-squares sense, to every camera's optical axis (camera_utils.py:144-156).

  With unit axis directions d_i through centres o_i the distance to axis i is |P_i (x - o_i)|, P_i = I - d_i d_i^T an
  orthogonal projector (P_i^T P_i = P_i), so the normal equations are (sum P_i) x = sum P_i o_i.
  """
  d = poses[:, :3, 2]
  o = poses[:, :3, 3]
  proj = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
  proj = np.einsum('nji,njk->nik', proj, proj)              # P^T P: equals P for unit d, kept general for un-normalised axes
  return np.linalg.solve(proj.sum(0), np.einsum('nij,nj->i', proj, o))


def transform_poses_pca(poses):
  """Scene normalisation for unbounded captures (what camera_utils.py:191-227 computes): rotate the principal axes of
  the camera centres onto x, y, z (largest spread first), keep the cameras' mean up-vector pointing to +z... i.e. a
  positive z component of the mean y axis, and scale the centres into [-1, 1]^3.  Returns (poses, 4x4 transform).

  A principal axis is only defined up to sign, and the two fix-ups below (handedness, up-vector) leave a 180-degree turn
  about z open.  Checkpoints and render paths are expressed in this frame, so the signs have to be the reference's: they are
  whatever LAPACK's general eigen-solver returns for the 3x3 scatter matrix of the centres, which is why this function asks
  the same solver the same question (`np.linalg.eig` of c^T c, camera_utils.py:205) instead of an SVD with a sign rule of its
  own (rounds 1-3: identical to the reference on 11 of the 12 captures of tests/golden/pca_poses.npz, diag(-1, -1, 1) off on
  one; now 12 of 12, tests/test_oracle_camera.py).
  """
  centres = poses[:, :3, 3]
  mean = centres.mean(0)
  c = centres - mean
  spread, vecs = np.linalg.eig(c.T @ c)
  axes = vecs[:, np.argsort(spread)[::-1]].T                              # rows: principal directions, largest spread first
  if np.linalg.det(axes) < 0:                                           # keep a right-handed frame
    axes[2] = -axes[2]
  world_to_pca = np.eye(4)
  world_to_pca[:3, :3] = axes
  world_to_pca[:3, 3] = -axes @ mean
  out = np.einsum('ij,njk->nik', axes, poses[:, :3, :4])
  out[:, :, 3] += world_to_pca[:3, 3]
  if out[:, 2, 1].mean() < 0:                                           # cameras upside down on average: turn about x
    turn = np.diag([1., -1., -1.])
    out = np.einsum('ij,njk->nik', turn, out)
    world_to_pca[:3] = turn @ world_to_pca[:3]
  shrink = 1.0 / np.abs(out[:, :, 3]).max()
  out[:, :, 3] *= shrink
  world_to_pca[:3] *= shrink
  return out, world_to_pca


# ----------------------------------------------------------------------------- render paths (host, NumPy float64)

NEAR_STRETCH = .9                 # push the near bound forward for the forward-facing path (camera_utils.py:154-156)
FAR_STRETCH = 5.                  # push the far bound back
FOCUS_DISTANCE = .75              # weight of the far bound, in disparity, in the focus depth

_F32_EPS = float(np.finfo(np.float32).eps)


def generate_spiral_path(poses, bounds, n_frames=120, n_rots=2, zrate=.5):
  """A forward-facing spiral (camera_utils.py:159-188): cameras circle in the average camera's x-y plane, with radii at the
  90th percentile of the capture positions, and all look at one point on the average optical axis.  Its depth is a
  weighted mean, in disparity, of the stretched near and far bounds."""
  near_bound = bounds.min() * NEAR_STRETCH
  far_bound = bounds.max() * FAR_STRETCH
  focal = 1 / ((1 - FOCUS_DISTANCE) / near_bound + FOCUS_DISTANCE / far_bound)
  radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), 90, 0), [1.]])
  cam2world = average_pose(poses)
  up = poses[:, :3, 1].mean(0)
  lookat = cam2world @ [0, 0, -focal, 1.]
  path = []
  for theta in np.linspace(0., 2. * np.pi * n_rots, n_frames, endpoint=False):
    position = cam2world @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.])
    path.append(viewmatrix(position - lookat, up, position))
  return np.stack(path, axis=0)


def _invert_step_cdf(t, log_w, n):
  """stepfun.sample(None, t, log_w, n) (stepfun.py:153-211, math.py:108-127): n points that split the mass of the step
  function (t [m + 1], weights softmax(log_w) [m]) evenly: the inverse CDF at u = linspace(0, 1 - eps32, n), no jitter."""
  w = np.exp(log_w - np.max(log_w))
  w = w / w.sum()
  cdf = np.concatenate([[0.], np.minimum(1., np.cumsum(w[:-1])), [1.]])
  u = np.linspace(0, 1. - _F32_EPS, n)
  last = len(cdf) - 1
  below = np.searchsorted(cdf, u, side='right') - 1             # the last knot with cdf <= u
  i0, i1 = np.clip(below, 0, last), np.clip(below + 1, 0, last)
  with np.errstate(divide='ignore', invalid='ignore'):
    frac = np.clip(np.nan_to_num((u - cdf[i0]) / (cdf[i1] - cdf[i0]), nan=0.), 0, 1)
  return t[i0] + frac * (t[i1] - t[i0])


def generate_ellipse_path(poses, n_frames=120, const_speed=True, z_variation=0., z_phase=0.):
  """An elliptical path around the captures' focus point (camera_utils.py:230-278): axes at the 90th percentile of the
  camera offsets, at height z = 0 (or, with z_variation, swinging between the 10th and 90th percentile of the capture
  heights); with const_speed the angles are resampled so that equal steps cover equal arc length."""
  center = focus_point_fn(poses)
  offset = np.array([center[0], center[1], 0])
  sc = np.percentile(np.abs(poses[:, :3, 3] - offset), 90, axis=0)
  low, high = -sc + offset, sc + offset
  z_low = np.percentile(poses[:, :3, 3], 10, axis=0)
  z_high = np.percentile(poses[:, :3, 3], 90, axis=0)

  def get_positions(theta):
    return np.stack([
        low[0] + (high - low)[0] * (np.cos(theta) * .5 + .5),
        low[1] + (high - low)[1] * (np.sin(theta) * .5 + .5),
        z_variation * (z_low[2] + (z_high - z_low)[2] * (np.cos(theta + 2 * np.pi * z_phase) * .5 + .5)),
    ], -1)

  theta = np.linspace(0, 2. * np.pi, n_frames + 1, endpoint=True)
  positions = get_positions(theta)
  if const_speed:
    lengths = np.linalg.norm(positions[1:] - positions[:-1], axis=-1)
    theta = _invert_step_cdf(theta, np.log(lengths), n_frames + 1)
    positions = get_positions(theta)
  positions = positions[:-1]                                    # the last one repeats the first
  avg_up = poses[:, :3, 1].mean(0)
  avg_up = avg_up / np.linalg.norm(avg_up)
  ind_up = np.argmax(np.abs(avg_up))
  up = np.eye(3)[ind_up] * np.sign(avg_up[ind_up])              # the world axis closest to the mean up vector
  return np.stack([viewmatrix(p - center, up, p) for p in positions])


def generate_interpolated_path(poses, n_interp, spline_degree=5, smoothness=.03, rot_weight=.1):
  """A smooth B-spline through keyframe poses (camera_utils.py:281-328): every pose becomes three points (position, a point
  rot_weight along the view axis, a point rot_weight along up), one spline goes through the nine coordinates, and the
  n_interp * (n - 1) samples are turned back into poses.  The degree falls back to n - 1 for few keyframes."""
  import scipy.interpolate
  pos = poses[:, :3, -1]
  points = np.stack([pos, pos - rot_weight * poses[:, :3, 2], pos + rot_weight * poses[:, :3, 1]], 1)
  n_key = points.shape[0]
  n = n_interp * (n_key - 1)
  tck, _ = scipy.interpolate.splprep(points.reshape(n_key, -1).T, k=min(spline_degree, n_key - 1), s=smoothness)
  new_points = np.array(scipy.interpolate.splev(np.linspace(0, 1, n, endpoint=False), tck)).T.reshape(n, 3, 3)
  return np.array([viewmatrix(p - l, u - p, p) for p, l, u in new_points])


def interpolate_1d(x, n_interp, spline_degree, smoothness):
  """camera_utils.py:331-340: a smoothing spline through a 1-D signal, sampled n_interp times per interval."""
  import scipy.interpolate
  tck = scipy.interpolate.splrep(np.linspace(0, 1, len(x), endpoint=True), x, s=smoothness, k=spline_degree)
  return scipy.interpolate.splev(np.linspace(0, 1, n_interp * (len(x) - 1), endpoint=False), tck)


def create_render_spline_path(config, image_names, poses, exposures):
  """camera_utils.py:343-395: the spline path through the poses of the images named by Config.render_spline_keyframes (a
  directory of images, or a text file with one name per line).  Returns (keyframe indices, render poses, render exposures
  or None)."""
  import os
  if os.path.isdir(config.render_spline_keyframes):
    keyframe_names = sorted(os.listdir(config.render_spline_keyframes))
  else:
    with open(config.render_spline_keyframes, 'r', encoding='utf-8') as fp:
      keyframe_names = fp.read().splitlines()
  spline_indices = np.array([i for i, n in enumerate(image_names) if n in keyframe_names])
  render_poses = generate_interpolated_path(poses[spline_indices], n_interp=config.render_spline_n_interp,
                                            spline_degree=config.render_spline_degree,
                                            smoothness=config.render_spline_smoothness, rot_weight=.1)
  render_exposures = None
  if config.render_spline_interpolate_exposure:
    if exposures is None:
      raise ValueError('config.render_spline_interpolate_exposure is True but create_render_spline_path() was passed '
                       'exposures=None.')
    # (heavy smoothing: a flickering exposure is worse than a lagging one)
    log_exposure = interpolate_1d(np.log(exposures[spline_indices]), config.render_spline_n_interp, spline_degree=5, smoothness=20)
    render_exposures = np.exp(log_exposure)
  return spline_indices, render_poses, render_exposures
