"""Geometry out of a trained model: the density on a regular grid, its isosurface as a triangle mesh, vertex colours, PLY.

  density_grid   the field of a density function on a box, queried chunk by chunk on the device
  extract_mesh   density_grid of `model.query_density`, ops.marching_tetrahedra (csrc/mesh.hip), colours from `model.nerf_hp`
  world_to_pixel the [3,4] projection of a perspective camera that csrc/tsdf.hip reads
  camera_record / project_points   any camera model the other way round, world point -> pixel: the packed record of the forward
                 model with its fold-back guard, and points through it on the device (csrc/camera_project.h)
  TsdfVolume     a truncated signed distance volume: integrate depth images (ops.tsdf_integrate, csrc/tsdf.hip), mesh its zero set
  tsdf_mesh      render the cameras of a dataset and fuse their depth into a TsdfVolume
  write_ply / read_ply   binary_little_endian 1.0
  mesh_stats     counts, Euler characteristic, open and non-manifold edges, signed volume, area (host, float64)
  filter_components / component_stats   connected components (ops.mesh_components, csrc/meshclean.hip): drop the small ones
  simplify       vertex clustering on a coarser grid with quadric-error placement (csrc/meshclean.hip)
  bake_texture   a texture atlas of per-face charts, every texel queried with its own footprint's Gaussian (csrc/atlas.hip)
  write_obj      OBJ + MTL + PNG of a mesh with a baked texture (write_ply takes the texture too)
  render_mesh    a mesh seen by a camera: face ids, depth, barycentrics, normals, colour; rasterised (csrc/raster.hip) for a pinhole,
                 ray cast (csrc/meshray.hip) for any camera model: lens distortion, fisheye, NDC datasets, panoramas
  cast_rays      what does this ray hit: the nearest intersection of free rays with a mesh (csrc/meshray.hip)
  sample_surface / point_mesh_distance / geometry_metrics   area-stratified surface samples, the distance of points to a mesh or
                 point cloud, and accuracy, completeness, Chamfer and F-score against a ground truth (csrc/meshdist.hip)
  closest_points / CropVolume / register   the closest point and normal on a mesh, Tanks and Temples' polygonal crop volumes, and
                 ICP refinement (point to surface with optional scale, point to plane) of a mesh against its ground truth
                 (csrc/meshreg.hip); geometry_metrics takes `crop`, `refine` and `normals`
  read_ply_geometry   a tolerant PLY reader for ground-truth meshes and point clouds

Grid convention (the kernels' own): field[i, j, k] sits at origin + spacing * (i, j, k), the linear point index is
(i * ny + j) * nz + k, and a point is inside iff field >= level.
"""

import math
import os
import time

import numpy as np
import torch

from multinerf_amd import _lib as L
from multinerf_amd import camera_utils, models, ops

# samples of one `mlp_call`: it keeps features, tangent rows and every layer's activations.  Measured for the 360 preset at
# full width (1024-wide NeRF MLP), profiles/mesh_extract.md: 3.0 GiB peak allocation at 2^18 samples, i.e. about 12 KiB a sample
# (profiles/mlp_call.md gives times at 2^20 samples per call but no memory figure).  2^18 keeps a query at a few GiB.
DEFAULT_CHUNK = 1 << 18


def grid_shape(bbox_min, bbox_max, resolution):
  """((nx, ny, nz), spacing) of the grid over a box.  The longest side gets exactly `resolution` points and sets the spacing,
  extent / (resolution - 1) rounded to float32 (what the kernels see).  Every other side gets the fewest points, at least 2,
  that reach its far face: ceil(q) + 1 with q = extent / longest extent * (resolution - 1), taken from the extents' ratio so that
  the rounding of the spacing cannot add a layer (a q within 1e-9 of an integer, relatively, counts as that integer).  The last
  point of a side may therefore fall short of the far face by the spacing's float32 rounding, a few 1e-8 of the extent."""
  lo, hi = [float(v) for v in bbox_min], [float(v) for v in bbox_max]
  resolution = int(resolution)
  if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi) or not all(h > l for l, h in zip(lo, hi)):
    raise ValueError(f'the box {lo} .. {hi} must have 3 finite coordinates a corner and a positive extent along every axis')
  if resolution < 2:
    raise ValueError(f'resolution = {resolution} must be at least 2')
  extent = [h - l for l, h in zip(lo, hi)]
  longest = max(extent)
  spacing = float(np.float32(longest / (resolution - 1)))
  shape = tuple(resolution if e == longest else max(2, int(math.ceil(e / longest * (resolution - 1) * (1. - 1e-9))) + 1) for e in extent)
  return shape, spacing


def grid_points(origin, spacing, shape, start, stop, device):
  """xyz [stop - start, 3] float32 of the grid points with linear indices start .. stop - 1: origin + spacing * float(index)."""
  _, ny, nz = shape
  idx = torch.arange(start, stop, dtype=torch.int64, device=device)
  ijk = torch.stack([idx // (ny * nz), (idx // nz) % ny, idx % nz], -1).to(torch.float32)
  o = torch.tensor(origin, dtype=torch.float32, device=device)
  return o + torch.tensor(spacing, dtype=torch.float32, device=device) * ijk


def density_grid(density_fn, bbox_min, bbox_max, resolution, std=0.5, chunk=DEFAULT_CHUNK, device='cuda'):
  """The field of `density_fn` on the regular grid over the box (`grid_shape`): returns (field [nx,ny,nz] float32 on the
  device, origin (3 floats) = bbox_min, spacing).  density_fn(xyz [n,3], std_world) -> [n] is called on `chunk` points at a
  time over the linear index range; for a model it is `lambda x, s: model.query_density(x[None], s)[0]`.  `std` is the
  standard deviation of the query's isotropic Gaussians in units of the spacing (std_world = std * spacing): the integrated
  positional encoding then pre-filters the field to the grid's resolution; std = 0 gives point samples."""
  shape, spacing = grid_shape(bbox_min, bbox_max, resolution)
  chunk = int(chunk)
  if chunk < 1:
    raise ValueError(f'chunk = {chunk} must be positive')
  origin = tuple(float(np.float32(v)) for v in bbox_min)
  n = shape[0] * shape[1] * shape[2]
  field = torch.empty((n,), dtype=torch.float32, device=device)
  for start in range(0, n, chunk):
    stop = min(start + chunk, n)
    d = density_fn(grid_points(origin, spacing, shape, start, stop, field.device), float(std) * spacing)
    field[start:stop] = d.reshape(stop - start)
  return field.reshape(shape), origin, spacing


def vertex_colors(model, verts, normals, std_world=0., chunk=DEFAULT_CHUNK):
  """uint8 [V,3] colours of surface points: the NeRF MLP's rgb at isotropic Gaussians around the vertices, seen head-on
  (view direction -normal, (0,0,1) where the normal is zero) with a zero GLO vector; viewdirs / glo_vec are passed only where
  the MLP reads them.  floor(clip(rgb, 0, 1) * 255 + 0.5)."""
  plan = model.nerf_plan
  V = int(verts.shape[0])
  out = torch.empty((V, 3), dtype=torch.uint8, device=verts.device)
  for start in range(0, V, int(chunk)):
    stop = min(start + int(chunk), V)
    m = stop - start
    vd = glo = None
    if plan.use_viewdirs:
      vd = -normals[start:stop]
      zero = (vd == 0).all(-1, keepdim=True)
      vd = torch.where(zero, torch.tensor([0., 0., 1.], dtype=vd.dtype, device=vd.device), vd).contiguous()
    if plan.glo > 0:
      glo = torch.zeros((m, plan.glo), dtype=torch.float32, device=verts.device)
    gaussians = models.points_to_gaussians(verts[start:stop, None, :], std_world)
    rgb = model.nerf_hp(None, gaussians, viewdirs=vd, glo_vec=glo)['rgb'].reshape(m, 3).to(torch.float32)
    out[start:stop] = torch.floor(torch.clamp(rgb, 0., 1.) * 255. + 0.5).to(torch.uint8)
  return out


def extract_mesh(model, bbox_min, bbox_max, resolution, density_threshold, std=0.5, chunk=DEFAULT_CHUNK, colors=True):
  """The isosurface density = density_threshold of the model's NeRF level inside a box, as
  dict(vertices [V,3] float32, normals [V,3] float32, faces [T,3] int32, colors [V,3] uint8 or None) of device tensors.

  The density is `model.query_density` on the grid of `density_grid` (`resolution` points along the longest side, Gaussians
  of `std` grid spacings), the surface ops.marching_tetrahedra (watertight and consistently oriented inside the box, open
  where the surface leaves it; normals point toward lower density), the colours `vertex_colors`.  `model` is built and bound
  (`construct_model`, or train_utils.setup_model + a restored checkpoint).  The preconditions of `Model.mlp_call` apply: it
  is inference only, each chunk is evaluated at once (a few KiB per sample: lower `chunk` on a crowded device), and it re-packs
  the bound parameters into the operand images a pending backward pass reads, so between a training forward pass and its
  backward pass it may run only on the parameters that pass ran on."""
  field, origin, spacing = density_grid(lambda x, s: model.query_density(x[None], s)[0], bbox_min, bbox_max, resolution,
                                        std=std, chunk=chunk, device=model.device)
  verts, normals, faces = ops.marching_tetrahedra(field, float(density_threshold), origin, spacing)
  cols = None
  if colors:
    cols = vertex_colors(model, verts, normals, float(std) * spacing, chunk)
  return dict(vertices=verts, normals=normals, faces=faces, colors=cols)


def world_to_pixel(pixtocam, camtoworld, distortion_params=None, pixtocam_ndc=None, camtype=camera_utils.ProjectionType.PERSPECTIVE):
  """The [3,4] float32 matrix P (a host array) with P @ (X, 1) = (u zc, v zc, zc) for a world point X seen by a perspective
  camera: inv(pixtocam) @ diag(1, -1, -1) @ [R^T | -R^T o] with camtoworld = [R | o], computed in float64.  Pixel px covers
  u in [px, px + 1), its centre is px + 0.5.

  zc is the rendered distance.  camera_utils.pixels_to_rays (the reference's internal/camera_utils.py:560-610) builds the ray
  of pixel (px, py) as directions = R diag(1, -1, -1) pixtocam (px + .5, py + .5, 1): for a perspective camera the last row of
  pixtocam is (0, 0, 1), so the camera-space z of `directions` is -1 (it is NOT normalised), and the distance_mean /
  distance_median a model renders along `directions` are exactly the zc of this matrix at the surface point: depth images
  and projection agree without a conversion.

  That holds for the undistorted pinhole model only, so everything else is refused with a ValueError: lens distortion
  parameters, an NDC ray space (pixtocam_ndc), ProjectionType.FISHEYE, and the spherical 'pano' camera of render paths."""
  if distortion_params is not None:
    raise ValueError('world_to_pixel: distortion parameters are given: a distorted camera has no [3,4] projection matrix')
  if pixtocam_ndc is not None:
    raise ValueError('world_to_pixel: pixtocam_ndc is given: rays in NDC space are not the straight lines of a [3,4] projection')
  if isinstance(camtype, str) and camtype == 'pano':
    raise ValueError("world_to_pixel: the 'pano' camera is spherical: it has no [3,4] projection matrix")
  if camera_utils.ProjectionType(camtype) == camera_utils.ProjectionType.FISHEYE:
    raise ValueError('world_to_pixel: ProjectionType.FISHEYE: a fisheye camera has no [3,4] projection matrix')
  K = np.linalg.inv(_host(pixtocam, np.float64).reshape(3, 3))
  c2w = _host(camtoworld, np.float64)[..., :3, :4].reshape(3, 4)
  R, o = c2w[:, :3], c2w[:, 3]
  w2c = np.concatenate([R.T, -(R.T @ o)[:, None]], 1)
  return np.ascontiguousarray(K @ np.diag([1., -1., -1.]) @ w2c, dtype=np.float32)


def camera_is_pinhole(distortion_params=None, pixtocam_ndc=None, camtype=camera_utils.ProjectionType.PERSPECTIVE):
  """True iff `world_to_pixel` accepts the camera model: no lens distortion, no NDC ray space, neither fisheye nor 'pano'."""
  if distortion_params is not None or pixtocam_ndc is not None or (isinstance(camtype, str) and camtype == 'pano'):
    return False
  return camera_utils.ProjectionType(camtype) == camera_utils.ProjectionType.PERSPECTIVE


_DISTORTION_KEYS = ('k1', 'k2', 'k3', 'k4', 'p1', 'p2')


def _distortion(x, y, k):
  """The lens distortion of camera_utils and its Jacobian, float64: (xd, yd, dxd/dx, dxd/dy, dyd/dx, dyd/dy), the terms of the
  undistortion's residual and Jacobian (csrc/camera.hip's cam_undistort) without the target."""
  r = x * x + y * y
  d = 1. + r * (k[0] + r * (k[1] + r * (k[2] + r * k[3])))
  d_r = k[0] + r * (2. * k[1] + r * (3. * k[2] + r * 4. * k[3]))
  d_x, d_y = 2. * x * d_r, 2. * y * d_r
  return (d * x + 2. * k[4] * x * y + k[5] * (r + 2. * x * x), d * y + 2. * k[5] * x * y + k[4] * (r + 2. * y * y),
          d + d_x * x + 2. * k[4] * y + 6. * k[5] * x, d_y * x + 2. * k[4] * x + 2. * k[5] * y,
          d_x * y + 2. * k[5] * y + 2. * k[4] * x, d + d_y * y + 2. * k[5] * x + 6. * k[4] * y)


def _distort(x, y, k):
  return _distortion(x, y, k)[:2]


def _undistort(xd, yd, k, eps=1e-9, max_iterations=200):
  """camera_utils' Newton iteration from the distorted point (csrc/camera.hip's cam_undistort), in float64 and run until no
  coordinate moves by more than 1e-15 (or max_iterations)."""
  x, y = xd.copy(), yd.copy()
  for _ in range(max_iterations):
    bx, by, fx_x, fx_y, fy_x, fy_y = _distortion(x, y, k)
    fx, fy = bx - xd, by - yd
    den = fy_x * fx_y - fx_x * fy_y
    ok = np.abs(den) > eps
    safe = np.where(ok, den, 1.)
    sx, sy = np.where(ok, (fx * fy_y - fy * fx_y) / safe, 0.), np.where(ok, (fy * fx_x - fx * fy_x) / safe, 0.)
    x, y = x + sx, y + sy
    if max(np.abs(sx).max(), np.abs(sy).max()) <= 1e-15:
      break
  return x, y


def fold_back_guard(pixtocam, height, width, k, fisheye=False):
  """r2_max of a camera record: the largest squared radius x^2 + y^2 of the UNDISTORTED image-plane points that the image's border
  comes from, times 1.01^2, at most pi^2 for a fisheye camera (where the radius is the angle theta); float64 on the host.

  The distortion polynomial is not injective: beyond the image it folds back, and a point out there would project into the image,
  mirrored.  The forward model (include/mnerf.h) therefore accepts a point only with x^2 + y^2 <= r2_max.  The border is sampled at
  the pixel corners along the four image edges (1.01 covers the sampling between them), sent through pixtocam and undistorted
  with the ray model's own Newton iteration, run to convergence.  The radius has no interior maximum over the image's pre-image,
  so the guard drops nothing that is in the image.  Every sample, distorted forward again, must come back to within 1e-3 pixel
  (a converged one does to 1e-12, a failed one is off by pixels), and it must lie on the branch of the distortion that contains
  the optical axis: the distortion's Jacobian there has a positive determinant and a positive trace, as it has at the centre,
  where it is the identity.  (Past the fold the iteration can converge too, to the MIRRORED root on the far side of the axis,
  which distorts forward exactly but has a reflected Jacobian.)  Otherwise the image reaches past the region where the model can
  be inverted, and this raises ValueError."""
  P = _host(pixtocam, np.float64).reshape(3, 3)
  H, W = int(height), int(width)
  us, vs = np.arange(W + 1, dtype=np.float64), np.arange(H + 1, dtype=np.float64)
  u = np.concatenate([us, us, np.zeros_like(vs), np.full_like(vs, W)])
  v = np.concatenate([np.zeros_like(us), np.full_like(us, H), vs, vs])
  xd, yd = P[0, 0] * u + P[0, 1] * v + P[0, 2], P[1, 0] * u + P[1, 1] * v + P[1, 2]
  k = [float(c) for c in k]
  with np.errstate(all='ignore'):
    x, y = _undistort(xd, yd, k)
    bx, by, j00, j01, j10, j11 = _distortion(x, y, k)
    A = np.linalg.inv(P)
    du, dv = A[0, 0] * bx + A[0, 1] * by + A[0, 2] - u, A[1, 0] * bx + A[1, 1] * by + A[1, 2] - v
    err = np.max(np.hypot(du, dv))
    principal = bool(((j00 * j11 - j01 * j10 > 0.) & (j00 + j11 > 0.)).all())
  if err <= 1e-3 and not principal:
    raise ValueError(f'fold_back_guard: a point on the border of the {H} x {W} image undistorts to the mirrored branch of the distortion '
                     'model: the image reaches past the region where the distortion model can be inverted')
  if not (err <= 1e-3):
    raise ValueError(f'fold_back_guard: a point on the border of the {H} x {W} image comes back {err:.3g} pixels from where it started after '
                     'undistortion and distortion: the image reaches past the region where the distortion model can be inverted')
  r2 = float(np.max(x * x + y * y)) * 1.01 ** 2
  return min(r2, math.pi ** 2) if fisheye else r2


def camera_record(pixtocam, camtoworld, height, width, distortion_params=None, pixtocam_ndc=None,
                  camtype=camera_utils.ProjectionType.PERSPECTIVE):
  """The packed float32 record [_lib.CAM_REC] (a host array) of the FORWARD camera model, world point -> pixel, for
  ops.project_points and ops.tsdf_integrate_cam; include/mnerf.h states the layout and every operation: the world-to-camera rows
  diag(1,-1,-1) [R^T | -R^T o] of camtoworld = [R | o] (12), the first two rows of inv(pixtocam) (6), k1 .. k4, p1, p2 (6),
  `fold_back_guard` (1), the model, height, width.  Computed in float64, rounded once.

  It inverts the project's own rays: camera_utils.pixels_to_rays for a perspective or fisheye `camtype` with or without
  `distortion_params`, ops.spherical_rays for camtype = 'pano' (pixtocam and distortion_params are then not read).  Refused with a
  ValueError: an NDC ray space (pixtocam_ndc: the distance a model renders there is not a world distance, so there is nothing a
  world point's depth could be compared with), a pixtocam whose last row is not exactly (0, 0, 1) (the distorted ray model sets
  the ray's camera-space z to 1, i.e. assumes that row), a camtoworld whose R is not a rotation to 1e-4, and an image that reaches
  past the distortion model's invertible region (`fold_back_guard`)."""
  if pixtocam_ndc is not None:
    raise ValueError('camera_record: pixtocam_ndc is given: rays in NDC space are refused, the distance a model renders along them is '
                     'not a world distance')
  pano = isinstance(camtype, str) and camtype == 'pano'
  H, W = int(height), int(width)
  if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
    raise ValueError(f'camera_record: an image of [{H}, {W}]: both sides must lie in 1 .. 2^24')
  c2w = _host(camtoworld, np.float64)[..., :3, :4].reshape(3, 4)
  R, o = c2w[:, :3], c2w[:, 3]
  if not np.isfinite(c2w).all() or np.abs(R.T @ R - np.eye(3)).max() > 1e-4:
    raise ValueError('camera_record: the left 3 x 3 block of camtoworld must be a rotation (R^T R = 1 to 1e-4)')
  rec = np.zeros((L.CAM_REC,), np.float64)
  rec[0:12] = (np.diag([1., -1., -1.]) @ np.concatenate([R.T, -(R.T @ o)[:, None]], 1)).reshape(-1)
  rec[26], rec[27] = H, W
  if pano:
    rec[25] = L.CAM_MODEL['pano']
    return rec.astype(np.float32)
  fisheye = camera_utils.ProjectionType(camtype) == camera_utils.ProjectionType.FISHEYE
  P = _host(pixtocam, np.float64).reshape(3, 3)
  if not np.array_equal(P[2], [0., 0., 1.]):
    raise ValueError(f'camera_record: the last row of pixtocam is {P[2].tolist()}, not (0, 0, 1): the distorted ray model assumes that row')
  if not np.isfinite(P).all() or np.linalg.matrix_rank(P) < 3:
    raise ValueError('camera_record: pixtocam is singular or not finite')
  distortion_params = dict(distortion_params or {})
  unknown = sorted(set(distortion_params) - set(_DISTORTION_KEYS))
  if unknown:
    raise ValueError(f'camera_record: distortion_params has unknown keys {unknown}; known: {list(_DISTORTION_KEYS)}')
  k = [float(distortion_params.get(name, 0.)) for name in _DISTORTION_KEYS]
  rec[12:18] = np.linalg.inv(P)[:2].reshape(-1)
  rec[18:24] = k
  rec[24] = fold_back_guard(P, H, W, k, fisheye=fisheye)
  rec[25] = L.CAM_MODEL['fisheye' if fisheye else 'perspective']
  return rec.astype(np.float32)


def project_points(points, pixtocam, camtoworld, height, width, distortion_params=None, camtype=camera_utils.ProjectionType.PERSPECTIVE):
  """World points seen by any camera model: (uv [..,2] float32, s [..] float32, valid [..] bool) of `points` [..,3] (a device tensor,
  or a host array that is moved to 'cuda'), on the device (ops.project_points, csrc/camera.hip, through `camera_record`).  It is the
  inverse of the project's ray generators: origins + s directions of pixel (px, py) gives int(u) = px, int(v) = py and that s, the
  distance a model renders along the ray and the depth of render_mesh(method='raycast').  valid: in front of the camera model,
  inside the fold-back guard and on the image (pixel px covers [px, px + 1)); a 'pano' camera sees every point but its own eye."""
  rec = camera_record(pixtocam, camtoworld, height, width, distortion_params=distortion_params, camtype=camtype)
  p = points.to(torch.float32) if torch.is_tensor(points) else torch.as_tensor(np.asarray(points, np.float32)).to('cuda')
  if p.dim() < 1 or p.shape[-1] != 3:
    raise ValueError(f'project_points: points must be [..,3], are {tuple(p.shape)}')
  lead = tuple(p.shape[:-1])
  uv, s, valid = ops.project_points(p.reshape(-1, 3).contiguous(), rec)
  return uv.reshape(lead + (2,)), s.reshape(lead), valid.reshape(lead)


# the 7 edge directions of csrc/mesh.hip, by edge number
_EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


class TsdfVolume:
  """A truncated signed distance volume on the grid of `grid_shape` over a box (Curless-Levoy running averages): `tsdf`
  [nx,ny,nz] in [-1, 1] in units of the truncation distance (starts at 1), `weight` [nx,ny,nz] the number of observations
  (starts at 0), `color` [nx,ny,nz,3] (starts at 0; None with colors=False), all float32 on the device.  The truncation is
  `trunc_voxels` grid spacings: a decision, not a derived number (larger closes thin gaps and thickens thin structures; below
  about 2 the zero crossing is no longer bracketed on diagonal edges)."""

  def __init__(self, bbox_min, bbox_max, resolution, trunc_voxels=3.0, colors=True, device='cuda'):
    self.shape, self.spacing = grid_shape(bbox_min, bbox_max, resolution)
    self.origin = tuple(float(np.float32(v)) for v in bbox_min)
    self.trunc = float(np.float32(float(trunc_voxels) * self.spacing))
    if not (self.trunc > 0. and math.isfinite(self.trunc)):
      raise ValueError(f'trunc_voxels = {trunc_voxels} must be positive and finite')
    self.tsdf = torch.ones(self.shape, dtype=torch.float32, device=device)
    self.weight = torch.zeros(self.shape, dtype=torch.float32, device=device)
    self.color = torch.zeros(self.shape + (3,), dtype=torch.float32, device=device) if colors else None
    self.projection = None                                  # set by tsdf_mesh: which projection its frames went through

  def integrate(self, depth, proj=None, acc=None, rgb=None, acc_threshold=0.5, cameras=None):
    """Fuse one frame (depth [H,W], proj [3,4]) or a stack ([F,H,W], [F,3,4]): depth is zc along the rays of `world_to_pixel`'s
    camera (0, negative, infinite or NaN: no measurement), acc (optional) the rays' opacity, below `acc_threshold` an empty ray
    that marks what it crosses as free space, rgb [...,3] the colours (required with a colour volume, ignored without).

    cameras= takes the place of proj for a camera that has no [3,4] matrix: one `camera_record` ([_lib.CAM_REC]) or a stack of them,
    all of one model (ops.tsdf_integrate_cam); depth is then the distance along the camera's own rays, what a model renders and
    what render_mesh(method='raycast') returns.  Exactly one of proj and cameras is given."""
    if (proj is None) == (cameras is None):
      raise ValueError('TsdfVolume.integrate: exactly one of proj (a pinhole [3,4] matrix a frame) and cameras (a camera record a frame) is given')
    dev = self.tsdf.device
    to = lambda x: None if x is None else torch.as_tensor(x).to(device=dev, dtype=torch.float32)
    depth, proj, acc, rgb = to(depth), to(proj), to(acc), to(rgb)
    if cameras is not None:
      cameras = np.asarray(cameras.detach().cpu().numpy() if torch.is_tensor(cameras) else cameras, np.float32)
    if depth.dim() == 2:
      depth, proj, cameras = depth[None], (None if proj is None else proj[None]), (None if cameras is None else cameras[None])
      acc, rgb = (None if acc is None else acc[None]), (None if rgb is None else rgb[None])
    if self.color is None:
      rgb = None
    elif rgb is None:
      raise ValueError('TsdfVolume.integrate: a volume with colours needs rgb')
    c = lambda x: None if x is None else x.contiguous()
    if cameras is not None:
      ops.tsdf_integrate_cam(self.tsdf, self.weight, self.color, self.origin, self.spacing, self.trunc, cameras, c(depth), acc=c(acc),
                             rgb=c(rgb), acc_threshold=acc_threshold)
      return
    ops.tsdf_integrate(self.tsdf, self.weight, self.color, self.origin, self.spacing, self.trunc, c(proj), c(depth), acc=c(acc),
                       rgb=c(rgb), acc_threshold=acc_threshold)

  def field(self):
    """(field, valid): the field marching tetrahedra runs on, -tsdf where a voxel was observed and -1 elsewhere (inside, field >=
    0, is BEHIND the surface), and the mask of observed voxels."""
    valid = self.weight > 0
    return torch.where(valid, -self.tsdf, torch.full_like(self.tsdf, -1.)), valid

  def mesh(self):
    """The zero set of the fused distance between observed voxels, as the dict `extract_mesh` returns.  Normals point into free
    space and faces are counter-clockwise seen from there.  A vertex' colour is the colour volume interpolated along its grid
    edge with the edge's t = (0 - f0) / (f1 - f0) in float32, then floor(clip(c, 0, 1) * 255 + 0.5)."""
    field, valid = self.field()
    verts, normals, faces, edges = ops.marching_tetrahedra(field, 0., self.origin, self.spacing, valid=valid, return_edges=True)
    cols = None
    if self.color is not None:
      _, ny, nz = self.shape
      step = torch.tensor([dx * ny * nz + dy * nz + dz for dx, dy, dz in _EDGE_DIRS], dtype=torch.int64, device=field.device)
      p0 = edges[:, 0]
      p1 = p0 + step[edges[:, 1]]
      f, c = field.reshape(-1), self.color.reshape(-1, 3)
      f0, f1 = f[p0], f[p1]
      t = (0. - f0) / (f1 - f0)
      t = torch.where((t >= 0.) & (t <= 1.), t, torch.full_like(t, 0.5))[:, None]
      c0, c1 = c[p0], c[p1]
      d = t * (c1 - c0)
      cols = torch.floor(torch.clamp(c0 + d, 0., 1.) * 255. + 0.5).to(torch.uint8)
    return dict(vertices=verts, normals=normals, faces=faces, colors=cols)


def tsdf_mesh(model, params, dataset, config, bbox_min, bbox_max, resolution, trunc_voxels=3.0, depth_key='distance_median',
              acc_threshold=0.5, frame_stride=1, frames_per_call=8, colors=True, timings=None):
  """Render every `frame_stride`-th camera of `dataset` and fuse the rendered depth into a TsdfVolume over the box; returns
  (the mesh dict of TsdfVolume.mesh, the volume).

  The frames are rendered the way render.py renders them (train_utils.create_render_fn, models.render_image, rng=None) with
  the bound parameters `params` (the `variables` of construct_model / a restored state's params); `depth_key`
  ('distance_median' or 'distance_mean'), 'acc' and 'rgb' of `frames_per_call` frames are stacked and integrated in one call.
  Any camera model but an NDC ray space is fused: an undistorted pinhole (`camera_is_pinhole`) goes through `world_to_pixel` and
  the [3,4] kernel exactly as before; lens distortion, a fisheye lens and the spherical 'pano' render camera go through
  `camera_record` and ops.tsdf_integrate_cam, the rendered distance being the ray parameter either way.  The volume's `projection`
  says which ('pinhole matrix' or 'camera records (<model>)').  A dict passed as `timings` gets the seconds of 'render', 'fusion'
  and 'isosurface' (each bracketed by a device synchronisation)."""
  from multinerf_amd import train_utils
  if dataset.pixtocam_ndc is not None:                      # (the one place that says so: extract_mesh.py passes this message on)
    raise ValueError('tsdf_mesh: the dataset renders in an NDC ray space (forward_facing): the rendered distance is not a world distance, '
                     'so it cannot be fused into a world-space volume')
  if depth_key not in ('distance_median', 'distance_mean'):
    raise ValueError(f"tsdf_mesh: depth_key = {depth_key!r} must be 'distance_median' or 'distance_mean'")
  frame_stride, frames_per_call = int(frame_stride), int(frames_per_call)
  if frame_stride < 1 or frames_per_call < 1:
    raise ValueError('tsdf_mesh: frame_stride and frames_per_call must be positive')
  camtype = 'pano' if getattr(dataset, '_render_spherical', False) else dataset.camtype
  pixtocams = _host(dataset.pixtocams, np.float64)
  pinhole = camera_is_pinhole(dataset.distortion_params, None, camtype)
  volume = TsdfVolume(bbox_min, bbox_max, resolution, trunc_voxels=trunc_voxels, colors=colors, device=model.device)
  volume.projection = 'pinhole matrix' if pinhole else f'camera records ({camtype if isinstance(camtype, str) else camtype.value})'
  render_fn = train_utils.create_render_fn(model)
  seconds = dict(render=0., fusion=0., isosurface=0.)

  def timed(key, fn):
    if timings is None:
      return fn()
    torch.cuda.synchronize()
    t0 = time.time()
    r = fn()
    torch.cuda.synchronize()
    seconds[key] += time.time() - t0
    return r

  def flush(stack):
    if stack:
      depth, proj, acc, rgb = ((torch if torch.is_tensor(stack[0][n]) else np).stack([s[n] for s in stack], 0) for n in range(4))
      kw = dict(proj=proj) if pinhole else dict(cameras=proj)
      timed('fusion', lambda: volume.integrate(depth, acc=acc, rgb=rgb if colors else None, acc_threshold=acc_threshold, **kw))
    del stack[:]

  stack = []
  for idx in range(0, dataset.size, frame_stride):
    pixtocam = pixtocams if pixtocams.ndim == 2 else pixtocams[idx]
    if pinhole:
      proj = torch.as_tensor(world_to_pixel(pixtocam, dataset.camtoworlds[idx], distortion_params=dataset.distortion_params,
                                            pixtocam_ndc=dataset.pixtocam_ndc, camtype=camtype)).to(model.device)
    else:                                                   # (a host record: ops.tsdf_integrate_cam checks and uploads the stack)
      proj = camera_record(pixtocam, dataset.camtoworlds[idx], dataset.height, dataset.width, distortion_params=dataset.distortion_params,
                           camtype=camtype)
    rays = dataset.generate_ray_batch(idx).rays
    r = timed('render', lambda: models.render_image(lambda rng, chunk: render_fn(params, 1.0, None, chunk), rays, None, config,
                                                    verbose=False))
    stack.append((r[depth_key].to(torch.float32), proj, r['acc'].to(torch.float32),
                  r['rgb'].to(torch.float32)))
    if len(stack) == frames_per_call:
      flush(stack)
  flush(stack)
  result = timed('isosurface', volume.mesh)
  if timings is not None:
    timings.update(seconds)
  return result, volume


def _compact(m, keep_faces):
  """The mesh dict restricted to the faces of a bool mask: vertices no kept face refers to are removed, the faces re-indexed,
  the order of the surviving vertices and faces unchanged."""
  verts, faces = m['vertices'], m['faces']
  V = int(verts.shape[0])
  faces = faces[keep_faces]
  used = torch.zeros((V,), dtype=torch.bool, device=verts.device)
  used[faces.reshape(-1).long()] = True
  new_id = (torch.cumsum(used, 0, dtype=torch.int64) - 1).to(torch.int32)
  colors = m.get('colors')
  return dict(vertices=verts[used].contiguous(), normals=m['normals'][used].contiguous(),
              faces=new_id[faces.long()].reshape(-1, 3).contiguous(), colors=None if colors is None else colors[used].contiguous())


def _component_counts(m):
  """(labels [V] int32, faces per label [V] int64, vertices per label [V] int64) on the device."""
  V = int(m['vertices'].shape[0])
  faces = m['faces'].contiguous()
  labels = ops.mesh_components(faces, V)

  def count(ids):                                           # a sort, not torch.bincount: its atomics pile up on one bin where
    out = torch.zeros((V,), dtype=torch.int64, device=ids.device)                      # the mesh is one big component
    which, n = torch.unique(ids.long(), return_counts=True)
    out[which] = n
    return out

  return labels, count(labels[faces[:, 0].long()]), count(labels)


def filter_components(m, min_faces=0, keep_largest=0, return_labels=False):
  """The mesh dict without its small connected components.  A component (ops.mesh_components: vertices joined through face edges,
  named by its smallest vertex id) is kept iff it has at least `min_faces` faces and, with keep_largest > 0, is among the
  `keep_largest` components with the most faces (ties go to the smaller label).  The vertices of dropped components go, and so do
  vertices no face refers to; surviving vertices and faces keep their order, faces are re-indexed, normals and colours are
  carried along.  The criterion is a face COUNT (integers, exact); an area would need ordered float sums.
  return_labels=True adds `labels` [V] int32, the INPUT mesh's component labels."""
  min_faces, keep_largest = int(min_faces), int(keep_largest)
  if min_faces < 0 or keep_largest < 0:
    raise ValueError(f'filter_components: min_faces = {min_faces} and keep_largest = {keep_largest} must not be negative')
  labels, n_faces, _ = _component_counts(m)
  keep = (n_faces >= min_faces) & (n_faces > 0)
  if keep_largest > 0:
    order = torch.sort(n_faces, descending=True, stable=True).indices[:keep_largest]     # stable: equal counts in ascending label
    top = torch.zeros_like(keep)
    top[order] = True
    keep &= top
  out = _compact(m, keep[labels[m['faces'][:, 0].long()].long()])
  if return_labels:
    out['labels'] = labels
  return out


def component_stats(m):
  """dict(count, faces=[...], vertices=[...]) of the mesh's connected components on the host: their number (a vertex in no face
  is a component of its own, with 0 faces) and their face and vertex counts, ordered by descending face count, then label."""
  labels, n_faces, n_verts = _component_counts(m)
  ids = torch.nonzero(n_verts).reshape(-1)
  f, v = n_faces[ids], n_verts[ids]
  order = torch.sort(f, descending=True, stable=True).indices
  return dict(count=int(ids.shape[0]), faces=f[order].tolist(), vertices=v[order].tolist())


def simplify(m, cell, origin=None, return_map=False):
  """Vertex clustering with quadric-error placement (Lindstrom 2000, DeCoro-Tatarchuk 2007): one output vertex per occupied cell
  of a grid of cubes of side `cell` (world units, positive and finite) at `origin` (default: the per-axis minimum of the
  vertices, one read-back).  include/mnerf.h states the contract: the cell of a vertex is int(floor((x - origin) / cell)) in
  float32, clusters are ordered by (cx, cy, cz), a cluster's vertex minimises the area-weighted squared distance to the planes
  of every face that touches the cluster, regularised toward the members' centroid and confined to the cell (the centroid where
  the solve fails or leaves the cell), its normal is the normalised sum and its colour the rounded mean of the members'.  A
  face survives iff its three clusters are distinct and no earlier face is the same directed triple up to rotation; surviving
  faces keep their order and winding.  Returns a new mesh dict; return_map=True adds `map` [V] int32, vertex -> output vertex,
  and `fallback` [V'] bool, the clusters placed at their centroid.

  Limitations: vertex clustering does not preserve manifoldness (two sheets closer than a cell merge, an edge may end up with
  more than two faces), and a pair of coincident faces of OPPOSITE winding (a thin sheet collapsed onto itself) stays in.
  A vertex that is not finite, or a cell index outside [0, 2^21), raises ValueError.  The sorts, `unique`, scans and compaction
  are torch on the device; the read-backs are the origin, the smallest key and the sizes."""
  verts, normals, faces, colors = m['vertices'].contiguous(), m['normals'].contiguous(), m['faces'].contiguous(), m.get('colors')
  colors = None if colors is None else colors.contiguous()
  dev = verts.device
  V, T = int(verts.shape[0]), int(faces.shape[0])
  cell = ops.positive_f32('simplify', 'cell', cell)
  if V == 0:
    out = dict(vertices=verts.clone(), normals=normals.clone(), faces=torch.zeros((0, 3), dtype=torch.int32, device=dev),
               colors=None if colors is None else colors.clone())
    if return_map:
      out['map'], out['fallback'] = torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.bool, device=dev)
    return out
  if origin is None:
    origin = verts.min(0).values.tolist()
    if not all(math.isfinite(v) for v in origin):
      raise ValueError('simplify: a vertex is not finite')
  origin = [float(np.float32(v)) for v in (origin.tolist() if torch.is_tensor(origin) else origin)]
  keys = ops.mesh_cluster_keys(verts, origin, cell)
  worst = int(keys.min())
  if worst == L.MESH_KEY_NONFINITE:
    raise ValueError('simplify: a vertex is not finite')
  if worst == L.MESH_KEY_OUTSIDE:
    lo = (verts.min(0).values.double() - torch.tensor(origin, dtype=torch.float64, device=dev)).min().item()
    if lo < 0:
      raise ValueError(f'simplify: a vertex lies {-lo:.6g} below the origin {origin}: every vertex must be at or above it')
    extent = (verts.max(0).values.double() - torch.tensor(origin, dtype=torch.float64, device=dev)).max().item()
    raise ValueError(f'simplify: cell = {cell:.6g} puts a vertex beyond cell index 2^21 - 1; the smallest legal cell for this mesh '
                     f'and origin is {extent / (L.MESH_CELL_LIMIT - 1):.6g}')
  ukeys, vmap = torch.unique(keys, sorted=True, return_inverse=True)
  K = int(ukeys.shape[0])
  members = torch.sort(vmap, stable=True).indices.to(torch.int32)
  zero = torch.zeros((1,), dtype=torch.int64, device=dev)
  member_start = torch.cat([zero, torch.cumsum(torch.bincount(vmap, minlength=K), 0)])
  vmap = vmap.to(torch.int32)
  mapped, canon, incident, keep = ops.mesh_cluster_faces(faces, vmap, K)
  inc = incident.reshape(-1)                                 # face-major: a stable sort by cluster leaves face ids ascending
  at = torch.nonzero(inc >= 0).reshape(-1)
  inc = inc[at].long()
  cluster_faces = (at[torch.sort(inc, stable=True).indices] // 3).to(torch.int32)
  face_start = torch.cat([zero, torch.cumsum(torch.bincount(inc, minlength=K), 0)])
  out_v, out_n, out_c, fallback = ops.mesh_cluster_solve(verts, normals, colors, faces, ukeys, member_start, members, face_start, cluster_faces,
                                                  origin, cell)
  ids = torch.nonzero(keep).reshape(-1)                      # distinct clusters; then the lowest id of every directed triple
  if ids.shape[0] > 0:
    _, group = torch.unique(canon[ids], dim=0, return_inverse=True)
    first = torch.full((int(group.max()) + 1,), T, dtype=torch.int64, device=dev).scatter_reduce(0, group, ids, 'amin')
    ids = ids[first[group] == ids]
  out = dict(vertices=out_v, normals=out_n, faces=mapped[ids].contiguous(), colors=out_c)
  if return_map:
    out['map'], out['fallback'] = vmap, fallback != 0
  return out


def _device_mesh(m):
  """The geometry of the mesh dict `m` as the contiguous tensors the ops wrappers take."""
  return dict(vertices=m['vertices'].contiguous(), normals=m['normals'].contiguous(), faces=m['faces'].contiguous())


def _model_color_fn(model):
  """The `color_fn` of `bake_texture` for a model: the NeRF MLP's rgb at the samples' Gaussians, with a zero GLO vector."""
  plan = model.nerf_plan

  def color_fn(means, covs, normals, viewdirs):
    n = int(means.shape[0])
    vd = viewdirs if plan.use_viewdirs else None
    glo = torch.zeros((n, plan.glo), dtype=torch.float32, device=means.device) if plan.glo > 0 else None
    return model.nerf_hp(None, (means[:, None], covs[:, None]), viewdirs=vd, glo_vec=glo)['rgb']

  return color_fn


def sh_directions(sh_dirs=2):
  """dirs [D,3] float32 (a host array) of `bake_texture`'s sh_dirs: an angular tesselation t of the icosahedron
  (geopoly.generate_basis('icosahedron', t, remove_symmetries=False): 42 directions for 2, 92 for 3), or a caller's [D,3] array,
  normalised in float64 and rounded to float32."""
  if isinstance(sh_dirs, (int, np.integer)) and not isinstance(sh_dirs, bool):
    from multinerf_amd import geopoly
    d = np.asarray(geopoly.generate_basis('icosahedron', int(sh_dirs), remove_symmetries=False), dtype=np.float64)
  else:
    d = _host(sh_dirs, np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
      raise ValueError(f'sh_dirs must be a tesselation or a [D,3] array of directions, is an array of shape {d.shape}')
  if not 1 <= d.shape[0] <= L.SHTEX_MAX_DIRS:
    raise ValueError(f'sh_dirs: {d.shape[0]} directions: must lie in 1 .. {L.SHTEX_MAX_DIRS}')
  length = np.sqrt((d * d).sum(-1, keepdims=True))
  if not (np.isfinite(length).all() and (length > 0.).all()):
    raise ValueError('sh_dirs: every direction must be finite and not zero')
  return np.ascontiguousarray((d / length).astype(np.float32))


def _bake_sh_chunk(color_fn, layout, start, means, covs, normals, face, dirs, basis, degree, lam, chunk, sh):
  """The SH part of one `bake_texture` pass over the samples start .. start + n - 1: weights, the colour of every (texel, direction)
  pair that counts, the fit, and the scatter into sh [H,W,K,3].  Returns the number of colour queries."""
  n, D = int(means.shape[0]), int(dirs.shape[0])
  w = ops.shtex_weights(dirs, normals)
  pairs = torch.nonzero((w > 0) & (face >= 0)[:, None])      # [P,2]: (sample, direction), rows ascending
  rgb = torch.zeros((n, D, 3), dtype=torch.float32, device=means.device)   # a pair that is not queried is never read by the fit
  for p0 in range(0, int(pairs.shape[0]), chunk):
    s, k = pairs[p0:p0 + chunk, 0], pairs[p0:p0 + chunk, 1]
    got = color_fn(means[s].contiguous(), covs[s].contiguous(), normals[s].contiguous(), dirs[k].contiguous())
    rgb[s, k] = got.reshape(int(s.shape[0]), 3).to(torch.float32)
  coef = ops.shtex_fit(dirs, normals, rgb, degree, lam, basis=basis)
  # the texel of sample s in closed form (include/mnerf.h: s = cell c (c + 1) + Y (c + 1) + X)
  c, cols = layout['cell'], layout['cols']
  keep = torch.nonzero(face >= 0)[:, 0]
  s = keep + start
  cell, r = s // (c * (c + 1)), s % (c * (c + 1))
  sh[(cell // cols) * c + r // (c + 1), (cell % cols) * (c + 1) + r % (c + 1)] = coef[keep]
  return int(pairs.shape[0])


def bake_texture(m, color_fn=None, model=None, cell=8, filter=1.0, chunk=DEFAULT_CHUNK, cols=None, return_float=False, sh_degree=None,
                 sh_dirs=2, sh_lambda=1e-3, timings=None):
  """A texture atlas for the mesh dict `m` (vertices, normals, faces on the device): dict(texture [H,W,3] uint8, mask [H,W] uint8,
  uv [T,3,2] float32, layout[, texture_f32 [H,W,3] float32 with return_float]) of device tensors.

  The parameterisation is include/mnerf.h's contract (`ops.atlas_layout`): every face has a chart of its own, a right triangle of
  `cell` texels a side, two to a cell of (cell + 1) x cell texels, the cells in a regular grid of `cols` columns (default: roughly
  square).  It is closed-form, so two runs give the same atlas.  uv holds u, v of each face's three corners (v = 1 at the top
  row); a bilinear lookup anywhere inside a face's UV triangle reads only texels that face owns, so there are no seams and no
  padding.  mask is 255 on the texels a face owns and 0 elsewhere (an odd face count's spare half cell, a face with a vertex that is
  not finite); texture is 0 there.

  Every texel is coloured by color_fn(means [n,3], covs [n,3,3], normals [n,3], viewdirs [n,3]) -> rgb [n,3], called on `chunk`
  samples at a time (`ops.atlas_samples`): the Gaussian has the texel's position on its face as mean and `filter`^2 / 12 times
  the second moments of the texel's parallelogram as covariance (the integrated positional encoding then pre-filters the colour
  to the texel's footprint; filter = 0 gives point samples), viewdirs is minus the interpolated normal.  texture =
  floor(clip(rgb, 0, 1) * 255 + 0.5).  With model= the colour is `model.nerf_hp(None, (means[:, None], covs[:, None]), ...)['rgb']`
  with a zero GLO vector, viewdirs / glo_vec passed only where the MLP reads them, as in `vertex_colors`; the preconditions of
  `Model.mlp_call` apply: it is inference only, each chunk is evaluated at once (a few KiB a sample: lower `chunk` on a crowded
  device), and it re-packs the bound parameters into the operand images a pending backward pass reads, so between a training
  forward pass and its backward pass it may run only on the parameters that pass ran on.  Exactly one of color_fn and model is
  given.  A mesh without faces gives a 0 x 0 texture and launches nothing.

  View-dependent texture.  With sh_degree = L in 0 .. 2 the dict gains sh [H,W,K,3] float32, K = (L + 1)^2, sh_degree, sh_dirs
  [D,3] float32 and sh_queries (the number of colour queries the fit made); texture, mask and uv are baked as before, bit for
  bit.  Per texel, sh holds the real spherical-harmonic coefficients (csrc/shtex.hip; include/mnerf.h states basis, order and
  every operation) that fit, channel by channel,
  color_fn's colour at the D fixed world directions `sh_dirs` (`sh_directions`: an icosahedron tesselation, 2 gives 42 directions
  and 3 gives 92, or a [D,3] array), in weighted least squares with weight min(max(-d . n, 0), 1): a view direction points from the
  eye to the surface, so only the hemisphere a texel can be seen from counts, and only those (texel, direction) pairs are queried
  (half of them on an antipodal set), in sub-chunks of `chunk` pairs; `chunk` bounds the texels of a pass as before.  sh_lambda is
  a ridge on every coefficient but the constant, relative to the mean diagonal entry of the normal matrix.  Its default 1e-3 is a
  DECISION, not a derived number: the float64 solve does not need it (on 42 directions the weighted normal matrix of degree 2 has
  a condition number up to 6.5e3, of degree 1 up to 51), it damps the fit of a noisy MLP colour.  A texel that cannot be solved
  holds its weighted mean colour as a constant.  `render_mesh` evaluates sh at each pixel's own view direction.  `timings`, a
  dict, receives the seconds of the SH part under 'sh' (it costs a device synchronisation before and after that part of a pass).

  What this is not: charts are uniform per face (a sliver gets as many texels as a fat triangle), there is no chart merging (mip
  levels below 0 mix neighbouring cells), and, without sh_degree, the single head-on view direction bakes a specular lobe as seen
  along -normal.  The SH texture has degree at most 2 (a sharp highlight is blurred), a fixed world direction set, and no occlusion
  test for a direction: a texel in a crevice is also fitted to directions it is never seen from."""
  if (color_fn is None) == (model is None):
    raise ValueError('bake_texture: exactly one of color_fn and model must be given')
  if model is not None:
    color_fn = _model_color_fn(model)
  chunk = int(chunk)
  if chunk < 1:
    raise ValueError(f'bake_texture: chunk = {chunk} must be positive')
  if sh_degree is not None:
    if isinstance(sh_degree, bool) or int(sh_degree) != sh_degree or not 0 <= int(sh_degree) <= L.SHTEX_MAX_DEGREE:
      raise ValueError(f'bake_texture: sh_degree = {sh_degree!r} must be None or an integer in 0 .. {L.SHTEX_MAX_DEGREE}')
    sh_degree, sh_lambda = int(sh_degree), float(sh_lambda)
    if not (sh_lambda >= 0. and math.isfinite(sh_lambda)):
      raise ValueError(f'bake_texture: sh_lambda = {sh_lambda} must be finite and not negative')
    dirs_host = sh_directions(sh_dirs)
  m = _device_mesh(m)
  dev = m['vertices'].device
  T = int(m['faces'].shape[0])
  layout = ops.atlas_layout(T, cell, cols)
  ops.check_face_indices('bake_texture', m['faces'], m['vertices'].shape[0])   # once, not per chunk
  H, W, total = layout['H'], layout['W'], layout['n_samples']
  texture = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
  mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
  texture_f32 = torch.zeros((H, W, 3), dtype=torch.float32, device=dev) if return_float else None
  uv = ops.atlas_uvs(m, layout) if T > 0 else torch.zeros((0, 3, 2), dtype=torch.float32, device=dev)
  if sh_degree is not None:
    dirs = torch.from_numpy(dirs_host).to(dev)
    basis = torch.from_numpy(ops.sh_basis(dirs_host, sh_degree)).to(dev)
    sh = torch.zeros((H, W, (sh_degree + 1) ** 2, 3), dtype=torch.float32, device=dev)
    queries = 0
  for start in range(0, total, chunk):
    stop = min(start + chunk, total)
    means, covs, normals, viewdirs, face = ops.atlas_samples(m, layout, start, stop, filter=filter, check_faces=False)
    rgb = color_fn(means, covs, normals, viewdirs).reshape(stop - start, 3).to(torch.float32).contiguous()
    ops.atlas_store(m, layout, start, rgb, face, texture, mask, texture_f32, check_faces=False)
    if sh_degree is not None:
      if timings is not None:
        torch.cuda.synchronize()
        t0 = time.time()
      queries += _bake_sh_chunk(color_fn, layout, start, means, covs, normals, face, dirs, basis, sh_degree, sh_lambda, chunk, sh)
      if timings is not None:
        torch.cuda.synchronize()
        timings['sh'] = timings.get('sh', 0.) + time.time() - t0
  out = dict(texture=texture, mask=mask, uv=uv, layout=layout)
  if return_float:
    out['texture_f32'] = texture_f32
  if sh_degree is not None:
    out.update(sh=sh, sh_degree=sh_degree, sh_dirs=dirs, sh_queries=queries)
  return out


def projection_origin(proj):
  """The eye of a [3,4] projection P = [A | a4] (`world_to_pixel`): the point o with P (o, 1) = 0, o = -A^{-1} a4, 3 float64 values.
  For world_to_pixel's matrix that is camtoworld[:3, 3].  A singular or non-finite A has no such point: ValueError."""
  P = _host(proj, np.float64).reshape(3, 4)
  A, a4 = P[:, :3], P[:, 3]
  if not np.isfinite(P).all() or np.linalg.matrix_rank(A) < 3:
    raise ValueError('projection_origin: the left 3 x 3 block of proj is singular or not finite: the projection has no eye')
  return -np.linalg.solve(A, a4)


def render_mesh(m, pixtocam, camtoworld, height, width, texture=None, colors=None, near=0.05, bg=(1., 1., 1.), cull='none', supersample=1,
                proj=None, threshold=None, view_dependent=True, origin=None, method='raster', distortion_params=None, pixtocam_ndc=None,
                camtype=camera_utils.ProjectionType.PERSPECTIVE):
  """The mesh dict `m` (vertices, normals, faces on the device) seen by a perspective camera, rasterised on the device
  (ops.raster_visibility + ops.raster_shade, csrc/raster.hip; include/mnerf.h states the contract): dict(rgb [H,W,3], acc [H,W],
  face [h,w] int32, depth [h,w], bary [h,w,3], normals [h,w,3], proj [3,4] the host matrix that was rendered) of device tensors, float32
  unless stated.

  The camera goes through `world_to_pixel`, which refuses everything but an undistorted pinhole; proj= takes a ready [3,4] matrix
  instead (pixtocam and camtoworld are then ignored).  depth is zc, the distance the model renders along the rays of
  camera_utils.pixels_to_rays (0 where no face is hit), acc is 1 where a face is hit: together they are what TsdfVolume.integrate takes.
  Only surface with zc > near is seen.  face is -1, bary and normals are 0 and rgb is `bg` where nothing is hit.

  The colour is `texture`: the dict `bake_texture` returns, or dict(texture [Ht,Wt,3] uint8 or float32, uv [T,3,2]) (read_ply's
  texcoord), looked up bilinearly; or `colors` [V,3] uint8 or float32 (True: m['colors']) blended over the face; or, with neither, the
  shaded normal 0.5 + 0.5 n.  cull = 'back' drops faces seen from behind (counter-clockwise seen from the camera is front).

  supersample = k renders at h x w = k height x k width, the first two rows of the matrix scaled by k, and returns rgb and acc
  box-averaged to [height, width] (plain torch); the GEOMETRIC buffers (face, depth, bary, normals) stay at the rendered resolution
  [k height, k width], since averaging ids or depths across a silhouette means nothing.  A mesh without faces gives the background and
  launches nothing.  `threshold` is ops.raster_visibility's.

  A texture dict that carries `sh` (bake_texture(..., sh_degree=), or read_ply's texture_sh put there as a [Ht,Wt,K,3] array; float16
  is converted to float32 once) is VIEW-DEPENDENT: after the shading pass, ops.shtex_shade (csrc/shtex.hip) overwrites rgb, where a
  face is hit, with the texel's spherical harmonics evaluated at the unit direction from `origin` to the pixel's surface point.
  origin defaults to the eye: camtoworld[:3, 3], or with proj= `projection_origin(proj)`.  view_dependent=False, or a dict without
  sh, renders the plain texture exactly as before.  Supersampling follows either.

  method = 'raster' (the default) is the above; a camera that `world_to_pixel` refuses (distortion_params, pixtocam_ndc, a fisheye or
  'pano' camtype) fails with its message.  method = 'raycast' renders ANY camera model by casting the ray of every pixel centre at
  the mesh (ops.mesh_raycast + ops.raycast_shade, csrc/meshray.hip), then ops.shtex_shade as above.  The rays are the model's own,
  built on the device: camera_utils.pixels_to_rays for a perspective or fisheye `camtype`, with or without `distortion_params`, and
  ops.spherical_rays for camtype = 'pano'; pixtocam and camtoworld are needed (proj= is refused), the origin is the camera's eye.  It
  returns the same dict with proj = None: depth is t, the ray parameter of the hit in units of the length of `directions`, which is
  the distance a model renders along those rays for every camera type and equals zc for a pinhole (0 where nothing is hit, as
  above); acc is 1 on a hit; only surface with t > near is seen; cull is the same `front`.  supersample = k casts k x k rays a pixel:
  pixtocam diag(1 / k, 1 / k, 1) at k height x k width (a panorama is simply rendered at k height x k width).  With `pixtocam_ndc` the
  rays are taken BEFORE the NDC conversion, because the mesh lives in world space: depth is then the world-space ray parameter and
  NOT the distance the model renders in its NDC ray space.  method = 'auto' rasterises where `camera_is_pinhole` and casts rays
  otherwise."""
  height, width, k = int(height), int(width), int(supersample)
  if height < 1 or width < 1 or k < 1:
    raise ValueError(f'render_mesh: height = {height}, width = {width} and supersample = {k} must be at least 1')
  if method not in ('raster', 'raycast', 'auto'):
    raise ValueError(f"render_mesh: method = {method!r} must be 'raster', 'raycast' or 'auto'")
  if method == 'auto':
    method = 'raster' if camera_is_pinhole(distortion_params, pixtocam_ndc, camtype) else 'raycast'
  if method == 'raycast':
    return _render_mesh_raycast(m, pixtocam, camtoworld, height, width, texture, colors, near, bg, cull, k, proj, view_dependent, origin,
                                distortion_params, camtype)
  P = np.array(world_to_pixel(pixtocam, camtoworld, distortion_params, pixtocam_ndc, camtype) if proj is None else
               _host(proj, np.float32).reshape(3, 4), dtype=np.float32)
  use_sh = bool(view_dependent) and texture is not None and texture.get('sh') is not None
  if use_sh and origin is None:
    origin = _host(camtoworld, np.float64)[..., :3, 3].reshape(3) if proj is None else projection_origin(proj)
  if k > 1:
    P[:2] *= np.float32(k)
  h, w = k * height, k * width
  dm = _device_mesh(m)
  dev = dm['vertices'].device
  if colors is True:
    colors = m.get('colors')
  kw = dict(colors=None if colors is None else torch.as_tensor(colors).to(dev).contiguous())
  if texture is not None:
    kw.update(texture=torch.as_tensor(texture['texture']).to(dev).contiguous(), uv=torch.as_tensor(texture['uv']).to(device=dev, dtype=torch.float32).contiguous())
  bg = [float(v) for v in bg]
  if int(dm['faces'].shape[0]) == 0:
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=dev)
    out = dict(face=torch.full((h, w), -1, dtype=torch.int32, device=dev), depth=z(h, w), acc=z(h, w), bary=z(h, w, 3), normals=z(h, w, 3),
               rgb=torch.tensor(bg, dtype=torch.float32, device=dev).expand(h, w, 3).contiguous())
  else:
    vis = ops.raster_visibility(dm, P, h, w, near, cull=cull, threshold=threshold)
    out = ops.raster_shade(dm, P, vis, near, bg=bg, **kw)
    if use_sh:
      sh = torch.as_tensor(texture['sh']).to(device=dev, dtype=torch.float32).contiguous()
      ops.shtex_shade(dm, out['face'], out['bary'], kw['uv'], sh, origin, out['rgb'])
  if k > 1:
    out['rgb'] = out['rgb'].reshape(height, k, width, k, 3).mean((1, 3))
    out['acc'] = out['acc'].reshape(height, k, width, k).mean((1, 3))
  out['proj'] = P
  return out


def _render_mesh_raycast(m, pixtocam, camtoworld, height, width, texture, colors, near, bg, cull, k, proj, view_dependent, origin,
                         distortion_params, camtype):
  """render_mesh(method='raycast'): its docstring says what this does."""
  if proj is not None or pixtocam is None or camtoworld is None:
    raise ValueError("render_mesh: method = 'raycast' builds the camera's rays: it needs pixtocam and camtoworld and takes no proj")
  pano = isinstance(camtype, str) and camtype == 'pano'
  if not pano:
    camtype = camera_utils.ProjectionType(camtype)
  h, w = k * height, k * width
  dm = _device_mesh(m)
  dev = dm['vertices'].device
  c2w = torch.as_tensor(_host(camtoworld, np.float32)[..., :3, :4].reshape(3, 4)).to(dev)
  if pano:
    origins, directions = ops.spherical_rays(c2w, h, w)[:2]
  else:
    ptc = _host(pixtocam, np.float64).reshape(3, 3) @ np.diag([1. / k, 1. / k, 1.])
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.int32, device=dev), torch.arange(w, dtype=torch.int32, device=dev), indexing='ij')
    origins, directions = camera_utils.pixels_to_rays(xs, ys, torch.as_tensor(ptc, dtype=torch.float32).to(dev), c2w,
                                                      distortion_params=distortion_params, camtype=camtype)[:2]
  use_sh = bool(view_dependent) and texture is not None and texture.get('sh') is not None
  if origin is None:
    origin = _host(camtoworld, np.float64)[..., :3, 3].reshape(3)
  if colors is True:
    colors = m.get('colors')
  kw = dict(colors=None if colors is None else torch.as_tensor(colors).to(dev).contiguous())
  if texture is not None:
    kw.update(texture=torch.as_tensor(texture['texture']).to(dev).contiguous(), uv=torch.as_tensor(texture['uv']).to(device=dev, dtype=torch.float32).contiguous())
  t, face, bary = ops.mesh_raycast(origins.reshape(-1, 3).contiguous(), directions.reshape(-1, 3).contiguous(), dm['vertices'], dm['faces'],
                                   t_min=ops.positive_f32('render_mesh', 'near', near), cull=cull, order=ops.pixel_tile_order(h, w, dev))
  face, bary = face.reshape(h, w), bary.reshape(h, w, 3)
  out = ops.raycast_shade(dm, face, bary, bg=[float(v) for v in bg], **kw)
  if use_sh:
    sh = torch.as_tensor(texture['sh']).to(device=dev, dtype=torch.float32).contiguous()
    ops.shtex_shade(dm, face, bary, kw['uv'], sh, origin, out['rgb'])
  hit = face >= 0
  out.update(face=face, bary=bary, acc=hit.to(torch.float32), depth=torch.where(hit, t.reshape(h, w), torch.zeros((), dtype=torch.float32, device=dev)))
  if k > 1:
    out['rgb'] = out['rgb'].reshape(height, k, width, k, 3).mean((1, 3))
    out['acc'] = out['acc'].reshape(height, k, width, k).mean((1, 3))
  out['proj'] = None
  return out


def cast_rays(m, origins, directions, t_min=0., t_max=None, cull='none', grid=None):
  """What does this ray hit?  dict(t [..] float32, face [..] int32, bary [..,3], points [..,3], normals [..,3] float32) of the rays
  origins + t directions ([..,3] each, tensors or host arrays; directions are NOT normalised and t is in units of their length) against
  the mesh dict `m` (vertices and faces, tensors or host arrays), in the rays' leading shape: the nearest intersection with
  t_min < t <= t_max (ops.mesh_raycast, csrc/meshray.hip; include/mnerf.h states the watertight hit test), the face that is hit (the
  lowest id among equally near ones), the barycentrics of the hit on it, the point origins + t directions and the face's unit normal
  (b - a) x (c - a) / |.| (ops.mesh_face_normals; it does not depend on the side the ray comes from).  cull = 'back' ignores faces seen
  from behind.  On a miss: t = +inf, face = -1, bary and normals 0, and points is not finite.  `grid` is ops.mesh_grid_build's for a
  caller that casts many batches at one mesh.  t_max is the primitive of an occlusion test: a ray towards a point at parameter 1 is
  blocked iff it hits something with t_max just below 1."""
  verts, faces = _shape(m)
  o = torch.as_tensor(origins).to(device=verts.device, dtype=torch.float32)
  d = torch.as_tensor(directions).to(device=verts.device, dtype=torch.float32)
  if o.dim() < 1 or o.shape[-1] != 3 or o.shape != d.shape:
    raise ValueError(f'cast_rays: origins and directions must be [..,3] of one shape, are {tuple(o.shape)} and {tuple(d.shape)}')
  lead = tuple(o.shape[:-1])
  o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
  t, face, bary = ops.mesh_raycast(o, d, verts, faces, t_min=t_min, t_max=t_max, cull=cull, grid=grid)
  hit = face >= 0
  normals = torch.zeros_like(o)
  if faces.shape[0] > 0:
    normals = torch.where(hit[:, None], ops.mesh_face_normals(verts, faces)[face.long().clamp(min=0)], normals)
  return dict(t=t.reshape(lead), face=face.reshape(lead), bary=bary.reshape(lead + (3,)), points=(o + t[:, None] * d).reshape(lead + (3,)),
              normals=normals.reshape(lead + (3,)))


def _host(x, dtype):
  if x is None:
    return None
  if torch.is_tensor(x):
    x = x.detach().cpu().numpy()
  return np.ascontiguousarray(x, dtype=dtype)


_VERTEX_FIELDS = [(n, '<f4') for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')]
_COLOR_FIELDS = [(n, 'u1') for n in ('red', 'green', 'blue')]
_FACE_DTYPE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
_FACE_UV_DTYPE = np.dtype([('n', 'u1'), ('v', '<i4', (3,)), ('nt', 'u1'), ('t', '<f4', (6,))])
_FACE_PROPS = [['list', 'uchar', 'int', 'vertex_indices']]
_FACE_UV_PROPS = _FACE_PROPS + [['list', 'uchar', 'float', 'texcoord']]


def _texture_arrays(name, texture, n_faces):
  """(image [H,W,3] uint8, uv [T,3,2] float32) on the host of a `bake_texture` result."""
  image, uv = _host(texture['texture'], np.uint8), _host(texture['uv'], np.float32)
  if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] == 0 or image.shape[1] == 0:
    raise ValueError(f'{name}: the texture must be a non-empty [H,W,3] image, is {image.shape}')
  if uv.shape != (n_faces, 3, 2):
    raise ValueError(f'{name}: uv must be [{n_faces},3,2] (three corners a face), is {uv.shape}')
  return image, uv


def _write_png(path, image):
  from PIL import Image
  Image.fromarray(image, 'RGB').save(path, format='PNG')


SH_DTYPES = ('float16', 'float32')


def _sh_array(name, texture, image, sh_dtype):
  """sh [H,W,K,3] of a texture dict on the host in `sh_dtype`, or None when the dict carries none."""
  if texture.get('sh') is None:
    return None
  if sh_dtype not in SH_DTYPES:
    raise ValueError(f'{name}: sh_dtype = {sh_dtype!r} must be one of {SH_DTYPES}')
  sh = _host(texture['sh'], np.float32)
  if sh.ndim != 4 or sh.shape[:2] != image.shape[:2] or sh.shape[2] not in (1, 4, 9) or sh.shape[3] != 3:
    raise ValueError(f'{name}: sh must be [{image.shape[0]},{image.shape[1]},K,3] with K = 1, 4 or 9, is {sh.shape}')
  if sh_dtype == 'float16':
    sh = np.clip(sh, -65504., 65504.)
  return sh.astype(np.dtype(sh_dtype))


def write_ply(path, mesh, texture=None, sh_dtype='float16'):
  """dict(vertices, normals, faces[, colors]) (device or host arrays) as a PLY file, binary_little_endian 1.0: vertex
  properties x y z nx ny nz (float) and red green blue (uchar) when the mesh has colours; faces as `list uchar int vertex_indices`.

  With `texture` (the dict `bake_texture` returns) a face also carries `list uchar float texcoord`, u v of its three corners (the
  layout MeshLab writes and reads), the header names the image in `comment TextureFile <name>.png`, and the image is written as
  <path without extension>.png next to the file.  Without it the file is byte for byte the one written before textures existed.

  A texture with `sh` (bake_texture(..., sh_degree=)) also writes <path without extension>_sh.npy, the array [H,W,K,3], and the
  header line `comment TextureSH <name>_sh.npy <degree>` after the TextureFile line.  sh_dtype = 'float16' (the default) halves
  the bytes: a DECISION; each coefficient is rounded to the nearest float16, a relative error of up to 2^-11, and clipped to
  +-65504; 'float32' writes it as baked.  A texture without sh writes the file it wrote before."""
  verts, normals = _host(mesh['vertices'], np.float32).reshape(-1, 3), _host(mesh['normals'], np.float32).reshape(-1, 3)
  faces, colors = _host(mesh['faces'], np.int32).reshape(-1, 3), _host(mesh.get('colors'), np.uint8)
  if normals.shape != verts.shape or (colors is not None and colors.reshape(-1, 3).shape != verts.shape):
    raise ValueError('write_ply: normals and colors must have one row per vertex')
  fields = _VERTEX_FIELDS + (_COLOR_FIELDS if colors is not None else [])
  v = np.zeros((verts.shape[0],), dtype=np.dtype(fields))
  for c, n in enumerate(('x', 'y', 'z')):
    v[n] = verts[:, c]
    v['n' + n] = normals[:, c]
  if colors is not None:
    for c, n in enumerate(('red', 'green', 'blue')):
      v[n] = colors.reshape(-1, 3)[:, c]
  f = np.zeros((faces.shape[0],), dtype=_FACE_DTYPE if texture is None else _FACE_UV_DTYPE)
  f['n'] = 3
  f['v'] = faces
  header = ['ply', 'format binary_little_endian 1.0']
  if texture is not None:
    image, uv = _texture_arrays('write_ply', texture, faces.shape[0])
    png = os.path.splitext(path)[0] + '.png'
    f['nt'] = 6
    f['t'] = uv.reshape(-1, 6)
    header += [f'comment TextureFile {os.path.basename(png)}']
    sh = _sh_array('write_ply', texture, image, sh_dtype)
    if sh is not None:
      npy = os.path.splitext(path)[0] + '_sh.npy'
      header += [f'comment TextureSH {os.path.basename(npy)} {math.isqrt(sh.shape[2]) - 1}']
  header += [f'element vertex {verts.shape[0]}']
  header += [f'property {"uchar" if t == "u1" else "float"} {n}' for n, t in fields]
  header += [f'element face {faces.shape[0]}', 'property list uchar int vertex_indices']
  if texture is not None:
    header += ['property list uchar float texcoord']
  header += ['end_header']
  with open(path, 'wb') as fh:
    fh.write(('\n'.join(header) + '\n').encode('ascii'))
    fh.write(v.tobytes())
    fh.write(f.tobytes())
  if texture is not None:
    _write_png(png, image)
    if sh is not None:
      np.save(npy, sh)


def read_ply(path):
  """A file written by `write_ply` as dict(vertices [V,3] float32, normals [V,3] float32, faces [T,3] int32,
  colors [V,3] uint8 or None) of host arrays; a file with texture coordinates adds texcoord [T,3,2] float32 and texture_file,
  the name in its `comment TextureFile` line (None without one).  Where the header has a `comment TextureSH <file> <degree>` line
  and that file lies next to the PLY, texture_sh is its array [H,W,K,3] as float32 (converted once, here) and
  texture_sh_file its name."""
  with open(path, 'rb') as fh:
    data = fh.read()
  end = data.index(b'end_header\n') + len(b'end_header\n')
  lines = data[:end].decode('ascii').split('\n')
  if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
    raise ValueError(f'{path}: not a binary_little_endian 1.0 PLY file')
  counts, props, element, texture_file, texture_sh = {}, {}, None, None, None
  for line in lines[2:]:
    w = line.split()
    if w[:1] == ['element']:
      element = w[1]
      counts[element], props[element] = int(w[2]), []
    elif w[:1] == ['property']:
      props[element].append(w[1:])
    elif w[:2] == ['comment', 'TextureFile']:
      texture_file = line.split(None, 2)[2]
    elif w[:2] == ['comment', 'TextureSH'] and len(w) >= 4:
      texture_sh = (' '.join(w[2:-1]), int(w[-1]))
  fields = [(p[-1], {'float': '<f4', 'uchar': 'u1'}[p[0]]) for p in props.get('vertex', [])]
  if fields[:6] != _VERTEX_FIELDS or fields[6:] not in ([], _COLOR_FIELDS) or props.get('face') not in (_FACE_PROPS, _FACE_UV_PROPS):
    raise ValueError(f'{path}: not the layout write_ply writes')
  textured = props['face'] == _FACE_UV_PROPS
  V, T = counts['vertex'], counts['face']
  v = np.frombuffer(data, dtype=np.dtype(fields), count=V, offset=end)
  f = np.frombuffer(data, dtype=_FACE_UV_DTYPE if textured else _FACE_DTYPE, count=T, offset=end + V * v.dtype.itemsize)
  if T and not ((f['n'] == 3).all() and (not textured or (f['nt'] == 6).all())):
    raise ValueError(f'{path}: a face that is no triangle')
  col = lambda names: np.stack([v[n] for n in names], -1) if V else np.zeros((0, 3), dtype=v.dtype[names[0]])
  out = dict(vertices=col(('x', 'y', 'z')), normals=col(('nx', 'ny', 'nz')), faces=np.array(f['v'], dtype=np.int32).reshape(T, 3),
             colors=col(('red', 'green', 'blue')) if len(fields) > 6 else None)
  if textured:
    out['texcoord'], out['texture_file'] = np.array(f['t'], dtype=np.float32).reshape(T, 3, 2), texture_file
    npy = None if texture_sh is None else os.path.join(os.path.dirname(os.path.abspath(path)), texture_sh[0])
    if npy is not None and os.path.isfile(npy):
      sh = np.load(npy, allow_pickle=False)
      if sh.ndim != 4 or sh.shape[2] != (texture_sh[1] + 1) ** 2 or sh.shape[3] != 3 or sh.dtype not in (np.float16, np.float32):
        raise ValueError(f'{npy}: not the [H,W,{(texture_sh[1] + 1) ** 2},3] float16 or float32 array of a degree-{texture_sh[1]} texture')
      out['texture_sh'], out['texture_sh_file'] = np.ascontiguousarray(sh, dtype=np.float32), texture_sh[0]
  return out


def write_obj(path, mesh, texture, sh_dtype='float16'):
  """dict(vertices, normals, faces) with the dict `bake_texture` returns as a Wavefront OBJ: <path> with `v`, `vn` (one a vertex),
  3 T `vt` lines (u v of each face's corners: a vertex has one UV per face it is in) and `f v/vt/vn` lines, 1-based;
  <path without extension>.mtl with one material whose map_Kd is <path without extension>.png, the texture.  Vertex colours are
  not written: OBJ has no standard place for them.  A texture with `sh` also writes <path without extension>_sh.npy as `write_ply`
  does (sh_dtype likewise); OBJ and MTL have no place to name it, so both files are what they are without it and a reader finds
  the array by its name."""
  verts, normals = _host(mesh['vertices'], np.float32).reshape(-1, 3), _host(mesh['normals'], np.float32).reshape(-1, 3)
  faces = _host(mesh['faces'], np.int32).reshape(-1, 3)
  if normals.shape != verts.shape:
    raise ValueError('write_obj: normals must have one row per vertex')
  image, uv = _texture_arrays('write_obj', texture, faces.shape[0])
  sh = _sh_array('write_obj', texture, image, sh_dtype)
  base = os.path.splitext(path)[0]
  name = os.path.basename(base)
  num = lambda row: ' '.join(f'{float(x):.9g}' for x in row)
  lines = [f'mtllib {name}.mtl', f'o {name}']
  lines += ['v ' + num(r) for r in verts]
  lines += ['vn ' + num(r) for r in normals]
  lines += ['vt ' + num(r) for r in uv.reshape(-1, 2)]
  lines += ['usemtl material0']
  lines += ['f ' + ' '.join(f'{int(i) + 1}/{3 * t + k + 1}/{int(i) + 1}' for k, i in enumerate(row)) for t, row in enumerate(faces)]
  with open(path, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
  with open(base + '.mtl', 'w') as fh:
    fh.write('\n'.join(['newmtl material0', 'Ka 1 1 1', 'Kd 1 1 1', 'Ks 0 0 0', 'illum 1', f'map_Kd {name}.png']) + '\n')
  _write_png(base + '.png', image)
  if sh is not None:
    np.save(base + '_sh.npy', sh)


def mesh_stats(verts, faces):
  """dict(V, T, E, euler, boundary_edges, nonmanifold_edges, signed_volume, area) of a triangle mesh, on the host in float64.
  E counts undirected edges; euler = V - E + T; a boundary edge has one face, a non-manifold edge more than two;
  signed_volume = sum of det(v0, v1, v2) / 6, positive for a closed surface whose faces are counter-clockwise seen from
  outside."""
  v = _host(verts, np.float64).reshape(-1, 3)
  f = _host(faces, np.int64).reshape(-1, 3)
  V, T = int(v.shape[0]), int(f.shape[0])
  e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0), -1)
  uses = np.unique(e, axis=0, return_counts=True)[1] if T else np.zeros((0,), dtype=np.int64)
  a, b, c = (v[f[:, k]] for k in range(3))
  E = int(uses.shape[0])
  return dict(V=V, T=T, E=E, euler=V - E + T, boundary_edges=int((uses == 1).sum()), nonmanifold_edges=int((uses > 2).sum()),
              signed_volume=float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.),
              area=float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=-1).sum()))


# ----------------------------------------------------------------------------- geometry metrics (csrc/meshdist.hip)

def _shape(m, device='cuda'):
  """(verts [V,3] float32, faces [T,3] int32) on the device of a mesh or point-cloud dict of tensors or host arrays; a dict without
  `faces` (or with None) is a cloud."""
  verts = torch.as_tensor(m['vertices']).to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
  faces = m.get('faces')
  if faces is None:
    return verts, torch.zeros((0, 3), dtype=torch.int32, device=verts.device)
  return verts, torch.as_tensor(faces).to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()


def _cloud_faces(verts):
  """The faces (i, i, i) under which a point cloud is a mesh."""
  return torch.arange(verts.shape[0], dtype=torch.int32, device=verts.device)[:, None].expand(-1, 3).contiguous()


def sample_surface(m, n, seed=0):
  """dict(points [n,3] float32, face [n] int32): n points on the surface of `m`, stratified in the area: face k gets within 2 of
  n A_k / A of them (ops.mesh_sample; the contract is in include/mnerf.h, the areas and their running sum are float64).  Faces with an
  index outside the vertices, a corner that is not finite or no area get none.  A mesh without faces is a point cloud: its vertices
  come back as they are, `face` numbers them, and n is ignored."""
  verts, faces = _shape(m)
  if faces.shape[0] == 0:
    return dict(points=verts, face=torch.arange(verts.shape[0], dtype=torch.int32, device=verts.device))
  cum = torch.cumsum(ops.mesh_face_areas(verts, faces), 0)
  points, face = ops.mesh_sample(verts, faces, cum, n, seed)
  return dict(points=points, face=face)


def point_mesh_distance(points, m, max_dist=None, grid=None):
  """dict(distance [N] float32, face [N] int32): the distance of every point to the surface of `m` (a point cloud when it has no
  faces: the distance to its nearest point) and the face (point) that attains it: sqrt of ops.point_mesh_distance's d2 in float32.
  With `max_dist`, farther faces do not count; where none counts, distance = +inf and face = -1."""
  verts, faces = _shape(m)
  if faces.shape[0] == 0:
    faces = _cloud_faces(verts)
  points = torch.as_tensor(points).to(device=verts.device, dtype=torch.float32).reshape(-1, 3).contiguous()
  d2, face = ops.point_mesh_distance(points, verts, faces, max_dist=max_dist, grid=grid, check_faces=False)
  return dict(distance=torch.sqrt(d2), face=face)


def _vnormals(m, verts):
  """The per-vertex normals of a shape dict as [V,3] float32 on the device of `verts`, or None."""
  n = m.get('normals') if isinstance(m, dict) else None
  if n is None:
    return None
  n = torch.as_tensor(n).to(device=verts.device, dtype=torch.float32).reshape(-1, 3).contiguous()
  if n.shape != verts.shape:
    raise ValueError(f'normals must be [{verts.shape[0]},3] like the vertices, are {tuple(n.shape)}')
  return n


def closest_points(points, m, max_dist=None, grid=None):
  """dict(point [N,3] float32, normal [N,3] float32, distance [N] float32, face [N] int32): the closest point of the surface of `m`
  to every point, the unit normal of the face it lies on (for a point cloud with `normals`: the nearest point's normal,
  normalised; without: 0), and `point_mesh_distance`'s distance and face (ops.mesh_closest; include/mnerf.h: the point is the foot
  of the very term of the distance formula that gave the distance).  Where no face counts (`max_dist`) or the point is not
  finite: point = the query itself, normal = 0, distance = +inf, face = -1."""
  verts, faces = _shape(m)
  cloud = faces.shape[0] == 0
  if cloud:
    faces = _cloud_faces(verts)
  points = torch.as_tensor(points).to(device=verts.device, dtype=torch.float32).reshape(-1, 3).contiguous()
  d2, face = ops.point_mesh_distance(points, verts, faces, max_dist=max_dist, grid=grid, check_faces=False)
  x, nrm = ops.mesh_closest(points, face, verts, faces, vnormals=_vnormals(m, verts) if cloud else None)
  return dict(point=x, normal=nrm, distance=torch.sqrt(d2), face=face)


class CropVolume:
  """A polygonal prism: the crop volume of the Tanks and Temples evaluation (the JSON files next to its ground truth).  `polygon`
  is a list of corners, [m,2] in the plane orthogonal to `axis` ('X': (y, z), 'Y': (x, z), 'Z': (x, y)) or [m,3] xyz of which the
  orthogonal coordinate is ignored; the prism reaches from axis_min to axis_max along the axis, both ends included.  A point is
  inside iff the even-odd crossing count over the polygon's edges is odd (ops.crop_polygon, csrc/meshreg.hip, float64; the rule is
  stated in include/mnerf.h).  This is Open3D's SelectionPolygonVolume rule as far as it could be restated from memory: agreement
  with Open3D itself is UNVERIFIED."""

  AXES = {'X': 0, 'Y': 1, 'Z': 2}
  _UV = {0: (1, 2), 1: (0, 2), 2: (0, 1)}

  def __init__(self, polygon, axis, axis_min, axis_max):
    ax = self.AXES.get(str(axis).upper()) if not isinstance(axis, (int, np.integer)) else int(axis)
    if ax not in (0, 1, 2):
      raise ValueError(f'CropVolume: axis must be X, Y or Z (or 0, 1, 2), is {axis!r}')
    poly = np.asarray(_host(polygon, np.float64), dtype=np.float64)
    if poly.ndim != 2 or poly.shape[1] not in (2, 3):
      raise ValueError(f'CropVolume: polygon must be [m,2] or [m,3], is {poly.shape}')
    if poly.shape[1] == 3:
      poly = poly[:, list(self._UV[ax])]
    if not 3 <= poly.shape[0] <= L.CROP_MAX_POLYGON:
      raise ValueError(f'CropVolume: a polygon of {poly.shape[0]} corners: must have 3 .. {L.CROP_MAX_POLYGON}')
    lo, hi = float(axis_min), float(axis_max)
    if not (np.isfinite(poly).all() and math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
      raise ValueError('CropVolume: the polygon, axis_min and axis_max must be finite, with axis_min <= axis_max')
    self.polygon, self.axis, self.axis_min, self.axis_max = np.ascontiguousarray(poly), ax, lo, hi

  @classmethod
  def from_json(cls, path):
    """The crop file of the Tanks and Temples toolbox: the keys bounding_polygon (a list of xyz), orthogonal_axis, axis_min and
    axis_max; any other key is ignored.  One ValueError names every key that is missing."""
    import json
    with open(path) as f:
      d = json.load(f)
    keys = ('bounding_polygon', 'orthogonal_axis', 'axis_min', 'axis_max')
    missing = [k for k in keys if not isinstance(d, dict) or k not in d]
    if missing:
      raise ValueError(f'CropVolume.from_json: {path} lacks {", ".join(missing)}')
    return cls(d['bounding_polygon'], d['orthogonal_axis'], d['axis_min'], d['axis_max'])

  def contains(self, points):
    """bool [N]: which of the points [N,3] (rounded to float32, on the device) lie inside."""
    pts = torch.as_tensor(points)
    pts = pts.to(device=pts.device if pts.is_cuda else 'cuda', dtype=torch.float32).reshape(-1, 3).contiguous()
    poly = torch.from_numpy(self.polygon).to(pts.device)
    return ops.crop_polygon(pts, poly, self.axis, self.axis_min, self.axis_max) != 0


ICP_MODES = ('point', 'plane')


def _finite_4x4(name, M):
  M = np.asarray(_host(M, np.float64), dtype=np.float64).reshape(-1)
  if M.shape != (16,) or not np.isfinite(M).all():
    raise ValueError(f'{name} must be a finite 4 x 4 matrix')
  return M.reshape(4, 4)


def _rodrigues(w):
  th = float(np.linalg.norm(w))
  K = np.array([[0., -w[2], w[1]], [w[2], 0., -w[0]], [-w[1], w[0], 0.]])
  if th < 1e-12:
    return np.eye(3) + K
  return np.eye(3) + (math.sin(th) / th) * K + ((1. - math.cos(th)) / (th * th)) * (K @ K)


def icp_step(sums, centre, mode, with_scale=False):
  """The 4 x 4 float64 update of one ICP iteration from the 47 sums of ops.icp_sums (host, NumPy): 'point': Kabsch on the centred
  cross-covariance with the determinant fixed, Umeyama's scale with `with_scale`; 'plane': the 6 x 6 normal equations, the rotation
  by Rodrigues' formula about `centre`."""
  S, c = np.asarray(sums, dtype=np.float64), np.asarray(centre, dtype=np.float64)
  n = S[0]
  D = np.eye(4)
  if mode == 'point':
    mp, mx = S[1:4] / n, S[4:7] / n
    H = S[7:16].reshape(3, 3) / n - np.outer(mp, mx)           # sum (p - mp)(x - mx)^T / n
    U, sv, Vt = np.linalg.svd(H)
    sign = np.array([1., 1., 1. if np.linalg.det(Vt.T @ U.T) >= 0. else -1.])
    R = Vt.T @ np.diag(sign) @ U.T
    scale = 1.
    if with_scale:
      var = S[16] / n - mp @ mp
      if not var > 0.:
        raise ValueError('register: the inliers have no spread: no scale can be estimated')
      scale = float((sv * sign).sum() / var)
    D[:3, :3] = scale * R
    D[:3, 3] = (mx + c) - scale * R @ (mp + c)
  else:
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = S[20:41]
    A = A + np.triu(A, 1).T
    xi = np.linalg.lstsq(A, -S[41:47], rcond=1e-12)[0]
    R = _rodrigues(xi[:3])
    D[:3, :3] = R
    D[:3, 3] = c - R @ c + xi[3:]
  return D


def register(pred, gt, init=None, max_dist=None, mode='plane', with_scale=False, max_iters=30, rel_tol=1e-6, n_samples=200_000, seed=0,
             crop=None, timings=None):
  """ICP refinement of the pose of `pred` against `gt` (meshes, or point clouds: dicts without faces):
  dict(transform [4,4] float64 from pred's frame to gt's, fitness, inlier_rmse, iterations, history).

  `pred` is sampled once (`sample_surface`, n_samples, seed; a cloud is its own sample) and the samples outside `crop` (a CropVolume
  in gt's frame) after `init` (4 x 4, default the identity) are dropped; gt's grid is built once.  An iteration moves the samples by
  the current transform in float64 on the device, rounds once to float32, finds the nearest face within `max_dist`
  (ops.point_mesh_distance), the closest point and its normal (ops.mesh_closest) and the 47 sums over the inliers (ops.icp_sums,
  about the centre of gt's box), reads those back and solves on the host in float64 (`icp_step`); the update is composed on the left.
    mode 'point': point to surface.  Kabsch; with_scale adds Umeyama's scale.  Converges linearly along the surface.
    mode 'plane': point to plane, the 6 x 6 system, quadratic near the solution.  Needs normals: a cloud `gt` must carry `normals`.
  fitness = inliers / samples, inlier_rmse = sqrt(mean |p - x|^2) over the inliers, both OF the returned transform.  It stops when
  |fitness - previous| and |inlier_rmse - previous| both fall below rel_tol, or after max_iters updates.  `max_dist` (required) may
  be a sequence: the stages run in the order given (coarse to fine), each from the last one's transform, max_iters each.  `history`
  lists dict(stage, max_dist, iteration, fitness, inlier_rmse) of every evaluation; `iterations` counts the updates of all stages.
  ValueError: 'plane' with with_scale or without target normals, an `init` that is not finite, fewer than 6 inliers in a stage.

  What this is not: there is no voxel down-sampling (the samples are stratified in the area already), no initial alignment from
  camera trajectories and no global registration: a poor `init` converges to a wrong pose.  `timings`, a dict, receives the seconds
  of `move`, `query`, `closest_sums` (with the read-back) and `solve`, summed over the iterations."""
  name = 'register'
  if mode not in ICP_MODES:
    raise ValueError(f'{name}: mode must be one of {ICP_MODES}, is {mode!r}')
  if mode == 'plane' and with_scale:
    raise ValueError(f"{name}: mode 'plane' estimates no scale: use mode 'point' with with_scale")
  if max_dist is None:
    raise ValueError(f'{name}: max_dist is required (a distance, or a sequence of them, coarse to fine)')
  stages = [float(d) for d in (max_dist if isinstance(max_dist, (list, tuple, np.ndarray)) else [max_dist])]
  if not stages or not all(d > 0. and math.isfinite(d) for d in stages):
    raise ValueError(f'{name}: max_dist must be positive and finite, is {max_dist}')
  max_iters, n_samples = int(max_iters), int(n_samples)
  if max_iters < 0 or n_samples < 1:
    raise ValueError(f'{name}: max_iters = {max_iters} must not be negative and n_samples = {n_samples} must be positive')
  T = np.eye(4) if init is None else _finite_4x4(f'{name}: init', init).copy()
  if not np.array_equal(T[3], [0., 0., 0., 1.]):
    raise ValueError(f'{name}: init must be affine (last row 0 0 0 1)')
  gv, gf = _shape(gt)
  vnormals = None
  if gf.shape[0] == 0:
    vnormals = _vnormals(gt, gv)
    gf = _cloud_faces(gv)
    if mode == 'plane' and vnormals is None:
      raise ValueError(f"{name}: mode 'plane' needs normals: the target is a point cloud without `normals`")
  dev = gv.device
  clock = {}

  def timed(key, fn):
    if timings is None:
      return fn()
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    clock[key] = clock.get(key, 0.) + time.time() - t0
    return out

  src = sample_surface(pred, n_samples, seed)['points'].double()

  def move(M):
    A, t = torch.from_numpy(M[:3, :3].T.copy()).to(dev), torch.from_numpy(M[:3, 3].copy()).to(dev)
    return (src @ A + t).float().contiguous()

  if crop is not None:
    src = src[crop.contains(move(T))].contiguous()
  N = int(src.shape[0])
  grid = ops.mesh_grid_build(gv, gf)
  if N == 0 or grid['n_valid'] == 0:
    raise ValueError(f'{name}: nothing to register: {N} samples, {grid["n_valid"]} valid target faces')
  centre = [0.5 * (float(a) + float(b)) for a, b in zip(grid['origin'], grid['hi'])]
  sums = torch.empty((L.ICP_SUMS,), dtype=torch.float64, device=dev)
  history, updates = [], 0
  for stage, md in enumerate(stages):
    prev = None
    for it in range(max_iters + 1):
      q = timed('move', lambda: move(T))
      d2, face = timed('query', lambda: ops.point_mesh_distance(q, gv, gf, max_dist=md, grid=grid, check_faces=False))

      def closest_sums():
        x, nrm = ops.mesh_closest(q, face, gv, gf, vnormals=vnormals)
        return ops.icp_sums(q, x, nrm, (face >= 0).to(torch.uint8), centre, out=sums).cpu().numpy()
      S = timed('closest_sums', closest_sums)
      if S[0] < 6:
        raise ValueError(f'{name}: stage {stage} (max_dist {md:g}): {int(S[0])} of {N} samples have a correspondence: at least 6 are needed')
      fitness, rmse = float(S[0]) / N, math.sqrt(max(float(S[18]), 0.) / float(S[0]))
      history.append(dict(stage=stage, max_dist=md, iteration=it, fitness=fitness, inlier_rmse=rmse))
      if it == max_iters or (prev is not None and abs(fitness - prev[0]) < rel_tol and abs(rmse - prev[1]) < rel_tol):
        break
      prev = (fitness, rmse)
      t0 = time.time()
      T = icp_step(S, centre, mode, with_scale) @ T
      clock['solve'] = clock.get('solve', 0.) + time.time() - t0
      updates += 1
  if timings is not None:
    timings.update(clock)
  return dict(transform=T, fitness=history[-1]['fitness'], inlier_rmse=history[-1]['inlier_rmse'], iterations=updates, history=history)


# default thresholds of `geometry_metrics` as fractions of the ground truth's bounding-box diagonal
GEOMETRY_THRESHOLDS = (0.0025, 0.005, 0.01)


def geometry_metrics(pred, gt, n_samples=1_000_000, thresholds=None, max_dist=None, seed=0, transform=None, bbox=None, timings=None,
                     crop=None, refine=None, normals=False):
  """Geometric error of the mesh `pred` against the ground truth `gt` (a mesh, or a point cloud: a dict without faces) as a dict of
  Python floats.  Both surfaces are sampled (`sample_surface`, n_samples points each, seeds `seed` and `seed + 1`; a cloud is its
  own sample); d_acc is the distance of pred's samples to gt (point to triangle, or point to point for a cloud), d_comp that of
  gt's samples to pred (`point_mesh_distance`).
    accuracy = mean d_acc, completeness = mean d_comp, chamfer = (accuracy + completeness) / 2 (DTU's three numbers),
    accuracy_median, completeness_median,
    precision@t = mean(d_acc < t), recall@t = mean(d_comp < t), fscore@t = 2 P R / (P + R), 0 when P + R = 0 (Tanks and Temples),
    for every t of `thresholds`, written with %g; n_pred, n_gt the numbers of samples scored.
  The reductions are torch float64 on the device.

  Decisions.  `max_dist` CLAMPS the distances to it (and lets the search stop there).  DTU's evaluation drops such points instead;
  clamping keeps a floater visible in the mean, where dropping rewards it.  `thresholds` left at None are GEOMETRY_THRESHOLDS =
  0.25 %, 0.5 % and 1 % of the diagonal of gt's bounding box: scale-free, and of the order of the thresholds Tanks and Temples
  publishes for its scenes (3 to 15 mm on scenes of metres); pass the benchmark's own where there are such.
  `transform` is a 4 x 4 matrix from pred's frame to gt's, applied to pred's vertices in float64 on the host before anything else.
  `bbox` (x0, y0, z0, x1, y1, z1) drops the samples of both shapes outside that axis-aligned box of gt's frame; the distances are
  still taken to the whole of the other shape.
  `timings`, a dict, receives the seconds of `sample`, `grid` and `query` (each bracketed by a device synchronisation).

  Tanks and Temples' protocol (all three off by default, and then the dict and every bit in it are what they were without them):
  `crop`, a `CropVolume` (the benchmark's polygonal prism, `CropVolume.from_json`), drops the samples of both shapes outside it, after
  `transform`, like `bbox`.  `refine`, a dict of `register`'s arguments (at least max_dist), runs the ICP refinement from
  `transform` (inside `crop`, unless the dict brings its own) and scores with the refined transform, which is returned under the key
  `transform` as a [4,4] float64 array, the one entry that is not a float.  `normals=True` adds normal_consistency_acc,
  normal_consistency_comp and normal_consistency, their mean: the mean over the samples of |m_i . n_i|, m_i the unit normal of the
  face the sample was drawn from (a cloud's own `normals`, normalised) and n_i that of the closest face of the other shape
  (`closest_points`); only pairs with both normals non-zero count (NaN if there is none), and the keys are absent when either
  shape is a cloud without normals.  Not supported: voxel down-sampling, alignment from camera trajectories, global registration
  (see `register`)."""
  pv, pf = _shape(pred)
  gv, gf = _shape(gt)
  dev = gv.device
  if crop is not None and not isinstance(crop, CropVolume):
    raise ValueError('geometry_metrics: crop must be a CropVolume')
  if refine is not None:
    kw = dict(refine)
    kw.setdefault('crop', crop)
    kw.setdefault('init', transform)
    transform = register(pred, gt, **kw)['transform']
  pn, gn = (_vnormals(pred, pv), _vnormals(gt, gv)) if normals else (None, None)
  if transform is not None:
    M = _finite_4x4('geometry_metrics: transform', transform)
    if pn is not None and pf.shape[0] == 0:                   # a cloud's normals move with it: n A^-1 (row form of the inverse transpose)
      pn = torch.from_numpy((_host(pn, np.float64) @ np.linalg.inv(M[:3, :3])).astype(np.float32)).to(dev)
    h = _host(pv, np.float64) @ M[:3, :3].T + M[:3, 3]
    w = _host(pv, np.float64) @ M[3, :3] + M[3, 3]
    pv = torch.from_numpy((h / w[:, None]).astype(np.float32)).to(dev)
  if gv.shape[0] == 0 or pv.shape[0] == 0:
    raise ValueError('geometry_metrics: a shape without vertices')
  if max_dist is not None and not (float(max_dist) > 0. and math.isfinite(float(max_dist))):
    raise ValueError(f'geometry_metrics: max_dist = {max_dist} must be positive and finite')
  if thresholds is None:
    finite = gv[torch.isfinite(gv).all(1)].double()
    diag = float(torch.linalg.norm(finite.max(0).values - finite.min(0).values))
    thresholds = tuple(f * diag for f in GEOMETRY_THRESHOLDS)
  thresholds = [float(t) for t in thresholds]
  if not all(t > 0. and math.isfinite(t) for t in thresholds):
    raise ValueError(f'geometry_metrics: thresholds must be positive and finite, are {thresholds}')
  clock = {}

  def timed(key, fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    clock[key] = clock.get(key, 0.) + time.time() - t0
    return out

  shapes = {'pred': (pv, pf if pf.shape[0] else None), 'gt': (gv, gf if gf.shape[0] else None)}
  as_dict = lambda k: dict(vertices=shapes[k][0], faces=shapes[k][1])
  drawn = {k: timed('sample', lambda k=k: sample_surface(as_dict(k), n_samples, seed + (k == 'gt'))) for k in shapes}
  samples, drawn_face = {k: d['points'] for k, d in drawn.items()}, {k: d['face'] for k, d in drawn.items()}
  if bbox is not None:
    box = [float(v) for v in bbox]
    if len(box) != 6 or not all(math.isfinite(v) for v in box) or any(box[d] > box[d + 3] for d in range(3)):
      raise ValueError(f'geometry_metrics: bbox must be x0, y0, z0, x1, y1, z1 with x0 <= x1 ..., is {bbox}')
    lo, hi = torch.tensor(box[:3], device=dev), torch.tensor(box[3:], device=dev)
    inside = {k: ((p >= lo) & (p <= hi)).all(1) for k, p in samples.items()}
    samples, drawn_face = {k: p[inside[k]].contiguous() for k, p in samples.items()}, {k: f[inside[k]] for k, f in drawn_face.items()}
  if crop is not None:
    inside = {k: crop.contains(p) for k, p in samples.items()}
    samples, drawn_face = {k: p[inside[k]].contiguous() for k, p in samples.items()}, {k: f[inside[k]] for k, f in drawn_face.items()}
  if min(p.shape[0] for p in samples.values()) == 0:
    raise ValueError('geometry_metrics: no sample of a shape is left to score')
  vnorm = {'pred': pn, 'gt': gn}
  with_normals = normals and all(shapes[k][1] is not None or vnorm[k] is not None for k in shapes)
  dist, consistency = {}, {}
  for key, src, dst in (('acc', 'pred', 'gt'), ('comp', 'gt', 'pred')):
    v, f = shapes[dst]
    cloud = f is None
    f = _cloud_faces(v) if cloud else f
    grid = timed('grid', lambda: ops.mesh_grid_build(v, f))
    d2, face = timed('query', lambda: ops.point_mesh_distance(samples[src], v, f, max_dist=max_dist, grid=grid, check_faces=False))
    d = torch.sqrt(d2).double()
    dist[key] = d.clamp(max=float(max_dist)) if max_dist is not None else d
    if with_normals:
      n_i = ops.mesh_closest(samples[src], face, v, f, vnormals=vnorm[dst] if cloud else None)[1].double()
      sv, sf = shapes[src]
      own = torch.nn.functional.normalize(vnorm[src].double(), dim=1) if sf is None else ops.mesh_face_normals(sv, sf).double()
      m_i = own[drawn_face[src].long().clamp(min=0)]
      counted = (n_i != 0).any(1) & (m_i != 0).any(1) & torch.isfinite(m_i).all(1)
      consistency[key] = float((m_i * n_i).sum(1).abs()[counted].mean()) if bool(counted.any()) else float('nan')
  if timings is not None:
    timings.update(clock)
  out = dict(accuracy=float(dist['acc'].mean()), completeness=float(dist['comp'].mean()))
  out['chamfer'] = 0.5 * (out['accuracy'] + out['completeness'])
  out['accuracy_median'], out['completeness_median'] = float(dist['acc'].median()), float(dist['comp'].median())
  for t in thresholds:
    P, R = float((dist['acc'] < t).double().mean()), float((dist['comp'] < t).double().mean())
    out[f'precision@{t:g}'], out[f'recall@{t:g}'], out[f'fscore@{t:g}'] = P, R, (2. * P * R / (P + R) if P + R > 0. else 0.)
  out['n_pred'], out['n_gt'] = float(samples['pred'].shape[0]), float(samples['gt'].shape[0])
  if with_normals:
    out['normal_consistency_acc'], out['normal_consistency_comp'] = consistency['acc'], consistency['comp']
    out['normal_consistency'] = 0.5 * (consistency['acc'] + consistency['comp'])
  if refine is not None:
    out['transform'] = np.array(transform, dtype=np.float64)
  return out


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply_geometry(path):
  """A ground-truth PLY file, read tolerantly, as dict(vertices [V,3] float32, faces [T,3] int32 (T = 0: a point cloud), normals
  [V,3] float32 or None, colors [V,3] uint8 or None) of host arrays.  `ascii` and `binary_little_endian`; a `vertex` element with
  x y z as float or double, optionally nx ny nz and red green blue, and any other scalar properties, which are skipped; optionally a
  `face` element with `list uchar|char int|uint vertex_indices|vertex_index`, further scalar properties (skipped) and the
  `list uchar float texcoord` of `write_ply`.  Triangles only; elements after these are ignored.  Anything else raises ValueError
  and names what it met.  (`read_ply` reads `write_ply`'s own layout and is untouched.)"""
  with open(path, 'rb') as fh:
    data = fh.read()
  at = data.find(b'end_header')
  if not data.startswith(b'ply') or at < 0:
    raise ValueError(f'{path}: not a PLY file')
  end = data.index(b'\n', at) + 1
  lines = [l.strip() for l in data[:end].decode('ascii', 'replace').splitlines()]
  fmt = next((l.split()[1] for l in lines if l.startswith('format ')), None)
  if fmt not in ('ascii', 'binary_little_endian'):
    raise ValueError(f'{path}: format {fmt}: only ascii and binary_little_endian are read')
  elements = []
  for line in lines:
    w = line.split()
    if w[:1] == ['element']:
      elements.append((w[1], int(w[2]), []))
    elif w[:1] == ['property']:
      if not elements:
        raise ValueError(f'{path}: a property before any element')
      elements[-1][2].append(w[1:])
  names = [e[0] for e in elements]
  if 'vertex' not in names:
    raise ValueError(f'{path}: no vertex element')
  wanted = names[:max(names.index('vertex'), names.index('face') if 'face' in names else 0) + 1]
  tokens = data[end:].split() if fmt == 'ascii' else None
  pos, out = (0 if fmt == 'ascii' else end), {}
  for name, count, props in elements[:len(wanted)]:
    for p in props:
      if p[0] == 'list' and (name != 'face' or p[1] not in ('uchar', 'uint8', 'char', 'int8') or p[2] not in _PLY_TYPES):
        raise ValueError(f'{path}: element {name} has the list property `{" ".join(p)}`')
      if p[0] != 'list' and p[0] not in _PLY_TYPES:
        raise ValueError(f'{path}: element {name} has a property of type {p[0]}')
    fields = []
    for p in props:
      if p[0] != 'list':
        fields.append((p[1], '<' + _PLY_TYPES[p[0]]))
        continue
      if p[3] in ('vertex_indices', 'vertex_index'):
        if p[2] not in ('int', 'int32', 'uint', 'uint32'):
          raise ValueError(f'{path}: face indices of type {p[2]}')
        length = 3
      elif p[3] == 'texcoord':
        length = 6
      else:
        raise ValueError(f'{path}: element face has the list property `{" ".join(p)}`')
      fields += [('#' + p[3], 'u1'), (p[3], '<' + _PLY_TYPES[p[2]], (length,))]
    dtype = np.dtype(fields)
    width = sum(int(np.prod(f[2])) if len(f) > 2 else 1 for f in fields)
    if fmt == 'ascii':
      rows = tokens[pos:pos + count * width]
      if len(rows) != count * width:
        raise ValueError(f'{path}: element {name} ends early' + (' (only triangles are read)' if name == 'face' else ''))
      flat = np.array(rows, dtype=np.float64).reshape(count, width)
      rec, first = np.zeros((count,), dtype=dtype), 0
      for f in fields:
        k = int(np.prod(f[2])) if len(f) > 2 else 1
        rec[f[0]] = flat[:, first] if len(f) == 2 else flat[:, first:first + k]
        first += k
      pos += count * width
    else:
      if len(data) - pos < count * dtype.itemsize:
        if name == 'face':
          raise ValueError(f'{path}: the face element does not hold {count} triangles (only triangles are read)')
        raise ValueError(f'{path}: element {name} ends early')
      rec = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
      pos += count * dtype.itemsize
    if name == 'face':
      key = 'vertex_indices' if 'vertex_indices' in rec.dtype.names else 'vertex_index' if 'vertex_index' in rec.dtype.names else None
      if key is None:
        raise ValueError(f'{path}: the face element has no vertex_indices')
      sizes = rec['#' + key]
      if count and (sizes != 3).any():
        raise ValueError(f'{path}: a face with {int(sizes[sizes != 3][0])} vertices (only triangles are read)')
    out[name] = rec
  v = out['vertex']
  V = len(v)
  if not all(n in (v.dtype.names or ()) and v.dtype[n].kind == 'f' for n in ('x', 'y', 'z')):
    raise ValueError(f'{path}: the vertex element needs x y z as float or double, has {v.dtype.names}')
  col = lambda ns, dt: np.ascontiguousarray(np.stack([v[n] for n in ns], -1).astype(dt)) if V else np.zeros((0, 3), dtype=dt)
  has = lambda ns: all(n in v.dtype.names for n in ns)
  faces = np.zeros((0, 3), dtype=np.int32)
  if 'face' in out and len(out['face']):
    f = out['face']
    faces = np.ascontiguousarray(f['vertex_indices' if 'vertex_indices' in f.dtype.names else 'vertex_index'].astype(np.int64))
    if faces.min() < 0 or faces.max() >= V:
      raise ValueError(f'{path}: face indices {faces.min()} .. {faces.max()} outside the {V} vertices')
    faces = faces.astype(np.int32)
  return dict(vertices=col(('x', 'y', 'z'), np.float32), faces=faces, normals=col(('nx', 'ny', 'nz'), np.float32) if has(('nx', 'ny', 'nz')) else None,
              colors=col(('red', 'green', 'blue'), np.uint8) if has(('red', 'green', 'blue')) else None)
