"""TSDF fusion for any camera model on the GPU (-m gpu): mnr_tsdf_integrate_cam through ops.tsdf_integrate_cam against the NumPy
restatement (tests/project_ref.py: every frame looked at for every voxel) -- bit for bit for the perspective model with lens
distortion, over the decided voxels for fisheye and pano --, the fold-back guard in a fusion, an undistorted record against the
pinhole kernel, two analytic scenes through mesh.TsdfVolume, a ray-cast round trip, mesh.tsdf_mesh / extract_mesh.py on a small
model with a panorama render path, and the refusals."""

import functools
import os

import numpy as np
import pytest
import torch

from multinerf_amd import _lib, mesh, ops
from tests import project_ref as P
from tests import test_gpu_tsdf as G
from tests import tsdf_ref as T

pytestmark = pytest.mark.gpu

H, W = G.H, G.W
assert (H, W) == (P.H, P.W)
TRUNC, THRESHOLD = G.TRUNC, G.THRESHOLD
GRIDS = G.GRIDS
dev, bits, assert_same_volumes = G.dev, G.bits, G.assert_same_volumes


@functools.lru_cache(maxsize=None)
def cameras(model):
  """[3,28]: the records of tests/test_gpu_project.py's three cameras (outside the box, inside it, seeing half of it)."""
  if model == 'pano':
    return np.stack([P.record(None, c, 'pano') for c in P.poses()])
  if model == 'fisheye':
    return np.stack([P.record(K, c, 'fisheye', P.FISHEYE_DISTORTION) for K, c in zip(P.fisheye_intrinsics(), P.poses())])
  if model == 'pinhole':
    return np.stack([P.record(K, c) for K, c in zip(P.intrinsics(), P.poses())])
  return np.stack([P.record(K, c, 'perspective', P.DISTORTION) for K, c in zip(P.intrinsics(), P.poses())])


def inputs(shape, model, F):
  origin, spacing = G.grid_frame(shape)
  depth, acc, rgb = G.images(F, sum(shape) + F)
  return dict(origin=origin, spacing=spacing, depth=depth, acc=acc, rgb=rgb, cameras=np.stack([cameras(model)[f % 3] for f in range(F)]))


@functools.lru_cache(maxsize=None)
def case(shape, model='perspective', F=3, colors=True, batches=None):
  """(inputs, the float32 restatement's volumes, its branch counts): computed once, shared, never written to."""
  inp = inputs(shape, model, F)
  tsdf, weight, color = P.new_volume(shape, colors)
  stats = {}
  f0 = 0
  for n in (batches or (F,)):
    sl = slice(f0, f0 + n)
    P.integrate(tsdf, weight, color, inp['origin'], inp['spacing'], TRUNC, inp['cameras'][sl], inp['depth'][sl],
                acc=inp['acc'][sl] if colors else None, rgb=inp['rgb'][sl] if colors else None, acc_threshold=THRESHOLD, stats=stats)
    f0 += n
  for a in tuple(v for v in inp.values() if isinstance(v, np.ndarray)) + (tsdf, weight) + ((color,) if colors else ()):
    a.setflags(write=False)
  return inp, (tsdf, weight, color), stats


def run(shape, inp, colors=True, batches=None):
  """The kernel on the inputs of `case` -> (tsdf, weight, color) host arrays."""
  tsdf, weight, color = (dev(a) for a in T.new_volume(shape, colors))
  F = inp['depth'].shape[0]
  f0 = 0
  for n in (batches or (F,)):
    sl = slice(f0, f0 + n)
    ops.tsdf_integrate_cam(tsdf, weight, color, inp['origin'], inp['spacing'], TRUNC, inp['cameras'][sl], dev(inp['depth'][sl]),
                           acc=dev(inp['acc'][sl]) if colors else None, rgb=dev(inp['rgb'][sl]) if colors else None, acc_threshold=THRESHOLD)
    f0 += n
  return tuple(None if t is None else t.cpu().numpy() for t in (tsdf, weight, color))


# ---- perspective with lens distortion: bit for bit


@pytest.mark.parametrize('colors', [True, False], ids=['acc_rgb', 'bare'])
@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: 'x'.join(map(str, s)))
def test_distorted_perspective_against_the_restatement(shape, colors):
  inp, want, stats = case(shape, colors=colors)
  print(f'{shape}: {stats}')
  # every way through the steps is taken, the new one included: in front of the camera but outside the fold-back guard
  for branch in ('behind', 'guarded', 'off_image', 'no_measurement', 'occluded', 'near', 'far') + (('empty',) if colors else ()):
    assert stats[branch] > 0, branch
  assert (want[1] == 0).any() and (want[1] >= 2).any()
  assert_same_volumes(run(shape, inp, colors), want)


def test_more_frames_than_one_launch_stages():
  F = _lib.TSDF_MAX_FRAMES + 6
  shape = (9, 10, 11)
  inp, want, _ = case(shape, F=F)
  assert want[1].max() > _lib.TSDF_MAX_FRAMES / 3
  assert_same_volumes(run(shape, inp), want)
  assert_same_volumes(run(shape, inp, batches=(_lib.TSDF_MAX_FRAMES, 6)), want)       # 70 frames in one call = 64 followed by 6


def test_two_runs_agree_bit_for_bit():
  for model in ('perspective', 'fisheye', 'pano'):
    inp = inputs(GRIDS[0], model, 3)
    assert_same_volumes(run(GRIDS[0], inp), run(GRIDS[0], inp))


# ---- fisheye and pano: the float64 restatement over the decided voxels


def voxel_positions(shape, origin, spacing):
  i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing='ij')
  o = np.asarray(origin, np.float32)
  return np.stack([o[d] + np.float32(spacing) * idx.astype(np.float32) for d, idx in enumerate((i, j, k))], -1)


def delta_of(shape, inp):
  """Four times the float32 restatement's worst deviation from the float64 one at this grid's voxels, over the call's records."""
  xyz = voxel_positions(shape, inp['origin'], inp['spacing'])
  worst = dict(uv=0., s=0., lhs=0.)
  for rec in inp['cameras'][:3]:
    for k, v in P.deviation(rec, xyz).items():
      worst[k] = max(worst[k], v)
  return {k: 4. * v for k, v in worst.items()}


@functools.lru_cache(maxsize=None)
def reference64(shape, model, F=3):
  """(inputs, float64 volumes, decided voxels, undecided pairs, pairs on the image, delta) of the float64 restatement."""
  inp = inputs(shape, model, F)
  delta = delta_of(shape, inp)
  tsdf, weight, color = P.new_volume(shape, True, np.float64)
  decided, n_und, n_pairs = P.integrate(tsdf, weight, color, inp['origin'], inp['spacing'], TRUNC, inp['cameras'], inp['depth'], acc=inp['acc'],
                                        rgb=inp['rgb'], acc_threshold=THRESHOLD, dtype=np.float64, delta=delta)
  return inp, (tsdf, weight, color), decided, n_und, n_pairs, delta


def rounding_bound(F, delta):
  """tests/test_gpu_tsdf.test_batching's count of roundings, 2 F + 6 of 2^-24 each for F frames (24 at its 9), plus what an error of
  delta in s moves an observation t = (d - s) / trunc by."""
  return (2 * F + 6) * 2. ** -24 * 1.01 + delta['s'] / TRUNC


def compare_decided(got, want, decided, bound, label):
  gt, gw, gc = got
  wt, ww, wc = want
  assert decided.mean() > 0.9 and (ww[decided] > 0).any() and (ww[decided] >= 2).any()
  assert np.array_equal(gw[decided].astype(np.float64), ww[decided].astype(np.float64))
  seen = decided & (ww > 0)
  et = float(np.abs(gt[seen].astype(np.float64) - wt[seen]).max())
  ec = float(np.abs(gc[seen].astype(np.float64) - wc[seen]).max())
  print(f'{label}: {int(seen.sum())} decided observed voxels of {decided.size}, max |tsdf - reference| {et:.3e}, colour {ec:.3e} (bound {bound:.3e})')
  assert et <= bound and ec <= bound
  unseen = decided & (ww == 0)
  assert (gt[unseen] == 1).all() and (gc[unseen] == 0).all()


@pytest.mark.parametrize('model', ['fisheye', 'pano'])
@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: 'x'.join(map(str, s)))
def test_fisheye_and_pano_against_the_float64_restatement(shape, model):
  """Over the voxels whose (voxel, frame) pairs are all decided -- the float64 projection at least delta from a pixel edge and from
  the guard, |d - s +- trunc| at least delta -- the weights are equal and tsdf and colour agree within `rounding_bound`.  At most 1 %
  of the pairs on the image may be undecided, counted by the restatement."""
  inp, want, decided, n_und, n_pairs, delta = reference64(shape, model)
  print(f'{shape} {model}: delta uv {delta["uv"]:.3e} px, s {delta["s"]:.3e}, guard {delta["lhs"]:.3e}; {n_und} of {n_pairs} pairs on the '
        f'image undecided ({n_und / n_pairs:.3%})')
  assert n_pairs > 0 and n_und <= 0.01 * n_pairs
  compare_decided(run(shape, inp), want, decided, rounding_bound(3, delta), f'{shape} {model}')


@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: 'x'.join(map(str, s)))
def test_an_undistorted_record_against_the_pinhole_kernel(shape):
  """The same cameras as [3,4] matrices through mnr_tsdf_integrate and as undistorted records through the general kernel: two
  float32 evaluations of one projection, compared over the voxels the float64 restatement calls decided (each side has its own
  roundings: twice the count, and delta is the records' float32 deviation, which the matrix path shares in kind)."""
  inp, _, decided, n_und, n_pairs, delta = reference64(shape, 'pinhole')
  assert n_und <= 0.01 * n_pairs
  proj = np.stack([mesh.world_to_pixel(np.linalg.inv(K), c) for K, c in zip(P.intrinsics(), P.poses())])
  tsdf, weight, color = (dev(a) for a in T.new_volume(shape, True))
  ops.tsdf_integrate(tsdf, weight, color, inp['origin'], inp['spacing'], TRUNC, dev(proj), dev(inp['depth']), acc=dev(inp['acc']),
                     rgb=dev(inp['rgb']), acc_threshold=THRESHOLD)
  old = tuple(t.cpu().numpy().astype(np.float64) for t in (tsdf, weight, color))
  bound = 2. * (2 * 3 + 6) * 2. ** -24 * 1.01 + 2. * delta['s'] / TRUNC
  compare_decided(run(shape, inp), old, decided, bound, f'{shape} pinhole record')


# ---- the fold-back guard in a fusion


def test_fold_back_leaves_the_voxels_unobserved():
  """k1 = -0.3: voxels in front of the camera at an undistorted radius of 1.1 .. 3 would land in the image, mirrored, and take an
  observation from a constant depth image.  With the guard their weight stays 0; voxels inside the image's cone are observed."""
  c2w = T.look_at((0., 0., 3.))
  rec = P.record(T.intrinsics(30., 30., W / 2., H / 2.), c2w, 'perspective', dict(k1=-0.3))
  shape = (33, 33, 9)
  origin, spacing = (-4., -4., 0.), 0.25
  xyz = voxel_positions(shape, origin, spacing).astype(np.float64)
  cam = (xyz - c2w[:, 3]) @ c2w[:, :3] * np.array([1., -1., -1.])
  rho = np.hypot(cam[..., 0], cam[..., 1]) / cam[..., 2]
  folded, inside = (rho >= 1.1) & (rho <= 3.), rho <= 0.3
  assert folded.sum() > 500 and inside.sum() > 20
  tsdf, weight, _ = (dev(a) for a in T.new_volume(shape, False))
  ops.tsdf_integrate_cam(tsdf, weight, None, origin, spacing, 10., rec[None], torch.full((1, H, W), 2.5, device='cuda'))
  weight = weight.cpu().numpy()
  assert (weight[folded] == 0).all() and (weight[inside] == 1).all()
  # (not vacuous: with the guard opened, a good part of the folded voxels is written)
  opened = rec.copy()
  opened[24] = np.float32(1e30)
  tsdf, w2, _ = (dev(a) for a in T.new_volume(shape, False))
  ops.tsdf_integrate_cam(tsdf, w2, None, origin, spacing, 10., opened[None], torch.full((1, H, W), 2.5, device='cuda'))
  assert (w2.cpu().numpy()[folded] == 1).mean() > 0.05


# ---- analytic scenes through TsdfVolume


def test_fisheye_sphere_scene_through_tsdf_volume():
  """The sphere of tests/tsdf_ref.py seen by its 12 positions as fisheye cameras (96 x 96 pixels at 96 pixels a radian, the
  Euclidean distance as depth): the float64 restatement alone gives V 5262, T 10520, max |r - 0.6| 0.0393, volume ratio 0.9642."""
  scene = P.fisheye_sphere_scene()
  volume = mesh.TsdfVolume(*T.SPHERE_BOX, T.SPHERE_RES, trunc_voxels=T.SPHERE_TRUNC_VOXELS)
  volume.integrate(scene['depth'], cameras=scene['cameras'], acc=scene['acc'], rgb=scene['rgb'])
  got = {k: v.cpu().numpy() for k, v in volume.mesh().items()}
  stats = mesh.mesh_stats(got['vertices'], got['faces'])
  figures = T.check_sphere_mesh(got['vertices'], got['normals'], got['faces'], stats)
  assert abs(stats['V'] - 5262) <= 10 and abs(figures['volume_ratio'] - 0.9642) < 1e-3
  # one frame, then the rest: the same observations
  other = mesh.TsdfVolume(*T.SPHERE_BOX, T.SPHERE_RES, trunc_voxels=T.SPHERE_TRUNC_VOXELS)
  other.integrate(scene['depth'][0], cameras=scene['cameras'][0], acc=scene['acc'][0], rgb=scene['rgb'][0])
  other.integrate(scene['depth'][1:], cameras=scene['cameras'][1:], acc=scene['acc'][1:], rgb=scene['rgb'][1:])
  assert torch.equal(other.weight, volume.weight) and (other.tsdf - volume.tsdf).abs().max() <= 1e-5


def test_inside_out_scene_through_tsdf_volume():
  """The inside of a sphere of radius 0.8 seen by two pano cameras (64 x 128) near its centre: a handful of panoramas observes
  every voxel in front of the surface.  The float64 restatement alone gives V 9228, T 18452, max |r - 0.8| 0.0027, volume ratio
  -0.9969: free space is the inside, so the signed volume and the normals are reversed."""
  scene = P.inside_out_scene()
  volume = mesh.TsdfVolume(*T.SPHERE_BOX, T.SPHERE_RES, trunc_voxels=T.SPHERE_TRUNC_VOXELS)
  volume.integrate(scene['depth'], cameras=scene['cameras'], acc=scene['acc'], rgb=scene['rgb'])
  got = {k: v.cpu().numpy() for k, v in volume.mesh().items()}
  stats = mesh.mesh_stats(got['vertices'], got['faces'])
  figures = P.check_inside_out_mesh(got['vertices'], got['normals'], got['faces'], stats)
  assert abs(stats['V'] - 9228) <= 10 and abs(figures['volume_ratio'] + 0.9969) < 1e-3
  r = np.linalg.norm(voxel_positions(volume.shape, volume.origin, volume.spacing), axis=-1)
  weight = volume.weight.cpu().numpy()
  assert (weight[r < 0.8 - volume.spacing] == 2).all()      # every voxel in front of the surface, by both cameras
  assert (weight[r > 0.8 + volume.trunc + volume.spacing] == 0).all()


# ---- render a mesh through a fisheye lens and fuse it back


def test_raycast_round_trip():
  """The restatement's sphere mesh rendered from the 12 positions at 96 x 96, once as pinhole `raster` renders fused through the
  [3,4] kernel (the existing path: the bar) and once as fisheye `raycast` renders fused through the records; both results are
  scored against the source with mesh.geometry_metrics.  Fisheye pixels are coarser off the axis: the Chamfer distance may be
  at most 1.5 times the bar."""
  src = T.sphere_reference()['mesh']
  source = dict(vertices=dev(src['vertices']), normals=dev(src['normals']), faces=dev(src['faces'].astype(np.int32)), colors=None)
  n = 96
  pixtocam = np.linalg.inv(T.intrinsics(float(n), float(n), n / 2., n / 2.))
  chamfer = {}
  for label, kw in (('pinhole raster', dict(method='raster')), ('fisheye raycast', dict(method='raycast', camtype='fisheye'))):
    volume = mesh.TsdfVolume(*T.SPHERE_BOX, T.SPHERE_RES, trunc_voxels=T.SPHERE_TRUNC_VOXELS)
    for pos in T.sphere_cameras():
      c2w = T.look_at(pos)
      r = mesh.render_mesh(source, pixtocam, c2w, n, n, **kw)
      if kw['method'] == 'raster':
        volume.integrate(r['depth'], proj=r['proj'], acc=r['acc'], rgb=r['rgb'])
      else:
        volume.integrate(r['depth'], cameras=mesh.camera_record(pixtocam, c2w, n, n, camtype='fisheye'), acc=r['acc'], rgb=r['rgb'])
    fused = volume.mesh()
    assert int(fused['faces'].shape[0]) > 5000
    chamfer[label] = mesh.geometry_metrics(fused, source, n_samples=100_000)['chamfer']
  print(f'ray-cast round trip: chamfer {chamfer}')
  assert chamfer['fisheye raycast'] <= 1.5 * chamfer['pinhole raster']


# ---- a small model with a panorama render path, and the script

BINDS = G.BINDS + ['Config.render_path = True', "Config.render_camtype = 'pano'", 'Config.render_path_frames = 3',
                   'Config.render_resolution = (48, 24)']


@pytest.fixture(scope='module')
def model_case():
  from multinerf_amd import configs, datasets, models
  config = configs.load_preset('blender_256', BINDS)
  model, variables = models.construct_model(G.SEED, None, config, device='cuda')
  dataset = datasets.load_dataset('test', config.data_dir, config, device='cuda')
  # (acc_threshold = 0: no ray of the untrained model counts as empty, so every frame goes through the d - s comparison)
  result, volume = mesh.tsdf_mesh(model, variables, dataset, config, *G.BOX, G.RES, acc_threshold=0.)
  return dict(config=config, model=model, variables=variables, dataset=dataset, result=result, volume=volume)


def test_tsdf_mesh_is_the_renders_through_the_ops(model_case):
  from multinerf_amd import models, train_utils
  config, model, dataset, volume = (model_case[k] for k in ('config', 'model', 'dataset', 'volume'))
  assert dataset._render_spherical and dataset.size == 3 and (dataset.height, dataset.width) == (24, 48)
  assert volume.projection == 'camera records (pano)'
  render_fn = train_utils.create_render_fn(model)
  depth, acc, rgb, recs = [], [], [], []
  for idx in range(3):
    r = models.render_image(lambda rng, rays: render_fn(model_case['variables'], 1.0, None, rays), dataset.generate_ray_batch(idx).rays,
                            None, config, verbose=False)
    depth.append(r['distance_median'].float())
    acc.append(r['acc'].float())
    rgb.append(r['rgb'].float())
    recs.append(mesh.camera_record(None, dataset.camtoworlds[idx], 24, 48, camtype='pano'))
  RES = G.RES
  tsdf = torch.ones((RES,) * 3, device='cuda')
  weight, color = torch.zeros_like(tsdf), torch.zeros((RES,) * 3 + (3,), device='cuda')
  ops.tsdf_integrate_cam(tsdf, weight, color, G.BOX[0], volume.spacing, 3 * volume.spacing, np.stack(recs), torch.stack(depth).contiguous(),
                         acc=torch.stack(acc).contiguous(), rgb=torch.stack(rgb).contiguous(), acc_threshold=0.)
  assert torch.equal(tsdf, volume.tsdf) and torch.equal(weight, volume.weight) and torch.equal(color, volume.color)
  assert (weight > 0).any()
  field = torch.where(weight > 0, -tsdf, torch.full_like(tsdf, -1.))
  verts, normals, faces = ops.marching_tetrahedra(field, 0., G.BOX[0], volume.spacing, valid=weight > 0)
  result = model_case['result']
  assert torch.equal(verts, result['vertices']) and torch.equal(normals, result['normals']) and torch.equal(faces, result['faces'])
  print(f'pano model: V {len(verts)} T {len(faces)}, {int((weight == 0).sum())} of {weight.numel()} voxels never observed, '
        f'{int((tsdf < 1).sum())} with tsdf < 1')


def test_script(model_case, tmp_path):
  """extract_mesh.py --method tsdf on the panorama render path writes mesh.tsdf_mesh's bytes and says which projection it used."""
  from multinerf_amd import checkpoints, train_utils
  ck = str(tmp_path / 'ckpt')
  state, _ = train_utils.create_optimizer(model_case['config'], model_case['variables'])
  state.step = 7
  checkpoints.save_checkpoint(ck, model_case['model'], state, 7)
  args = ['--preset', 'blender_256']
  for b in BINDS + [f"Config.checkpoint_dir = '{ck}'"]:
    args += ['--gin_bindings', b]
  out = str(tmp_path / 'pano.ply')
  stdout = G.run_script(args + ['--resolution', str(G.RES), '--bbox', '-1,-1,-1,1,1,1', '--method', 'tsdf', '--tsdf_split', 'test', '--acc_threshold', '0', '--out', out])
  want = str(tmp_path / 'want.ply')
  mesh.write_ply(want, model_case['result'])
  assert open(out, 'rb').read() == open(want, 'rb').read()
  assert 'projection: camera records (pano)' in stdout and '3 frames of 24 x 48' in stdout


# ---- refusals


def test_refusals_leave_the_volumes_untouched():
  shape = (4, 4, 4)
  tsdf, weight, color = (dev(a) for a in T.new_volume(shape))
  recs = cameras('perspective')
  depth, rgb = torch.ones((3, H, W), device='cuda'), torch.ones((3, H, W, 3), device='cuda')
  call = lambda cams, d=depth, c=color, r=rgb, trunc=1.: ops.tsdf_integrate_cam(tsdf, weight, c, (0., 0., 0.), 1., trunc, cams, d, rgb=r)
  with pytest.raises(ValueError, match=r'\[3, 28\]'):         # a record stack of the wrong length
    call(recs[:2])
  with pytest.raises(ValueError, match=r'\[3, 28\]'):
    call(recs[:, :27])
  with pytest.raises(ValueError, match='one camera model'):
    call(np.stack([recs[0], cameras('fisheye')[1], recs[2]]))
  with pytest.raises(ValueError, match='another size'):
    call(recs, d=torch.ones((3, H + 1, W), device='cuda'), r=torch.ones((3, H + 1, W, 3), device='cuda'))
  with pytest.raises(ValueError, match='both given or both None'):
    call(recs, r=None)
  with pytest.raises(ValueError, match='trunc'):
    call(recs, trunc=0.)
  volume = mesh.TsdfVolume((-1., -1., -1.), (1., 1., 1.), 5, colors=False)
  for kw in (dict(), dict(proj=np.zeros((3, 3, 4), np.float32), cameras=recs)):      # neither, both
    with pytest.raises(ValueError, match='exactly one'):
      volume.integrate(depth, **kw)
  pixtocam, c2w = np.linalg.inv(P.intrinsics()[0]), P.poses()[0]
  with pytest.raises(ValueError, match='NDC'):
    mesh.camera_record(pixtocam, c2w, H, W, pixtocam_ndc=pixtocam)
  projective = pixtocam.copy()
  projective[2, 1] = -1e-5
  with pytest.raises(ValueError, match='last row'):
    mesh.camera_record(projective, c2w, H, W, camtype='fisheye')
  assert torch.equal(tsdf, torch.ones_like(tsdf)) and not weight.any() and not color.any()
  assert torch.equal(volume.tsdf, torch.ones_like(volume.tsdf)) and not volume.weight.any()
  ops.tsdf_integrate_cam(tsdf, weight, color, (0., 0., 0.), 1., 1., recs[:0], depth[:0], rgb=rgb[:0])      # no frames: a no-op
  assert not weight.any()
