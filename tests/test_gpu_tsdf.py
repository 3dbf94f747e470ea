"""TSDF fusion on the GPU (-m gpu): mnr_tsdf_integrate through ops.tsdf_integrate against the NumPy restatement
(tests/tsdf_ref.py: float32 in the kernel's order, every frame looked at for every voxel) bit for bit, batching, determinism,
the validity filter of ops.marching_tetrahedra, the analytic sphere scene through mesh.TsdfVolume, and
mesh.tsdf_mesh / extract_mesh.py on a small model."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import _lib, mesh, ops
from tests import mesh_ref as R
from tests import tsdf_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 20
TRUNC, THRESHOLD = 0.3, 0.5

# A workgroup owns a brick of 4 x 8 x 8 voxels: (5,6,70) has ragged bricks along every axis, (3,2,257) two dimensions smaller
# than a brick and 33 bricks along z, (9,10,11) 3 x 2 x 2 bricks of which 7 are ragged.
GRIDS = [(5, 6, 70), (3, 2, 257), (9, 10, 11)]


def grid_frame(shape):
  """(origin, spacing) of a grid centred on the world origin whose longest side spans [-1, 1], a little off the round numbers."""
  spacing = 2. / (max(shape) - 1)
  return tuple(-0.5 * spacing * (n - 1) + off for n, off in zip(shape, (0.013, -0.02, 0.007))), spacing


def cameras():
  """[3,3,4] float32: a camera with fx != fy and an off-centre principal point that sees the whole grid; one INSIDE the box
  (voxels behind it have zc <= 0); one whose frustum misses about half of the box."""
  K = T.intrinsics(15., 15., W / 2., H / 2.)
  return np.stack([T.projection(T.intrinsics(13., 17., 8.7, 13.1), T.look_at((2.1, 1.7, 1.3))),
                   T.projection(K, T.look_at((0.01, 0.02, 0.3), target=(0.3, -0.2, 1.))),
                   T.projection(K, T.look_at((3., 0.2, 0.1), target=(0., 0., 1.6)))])


def images(F, seed):
  """depth [F,H,W] in [0.5, 4] with planted 0, inf, NaN and negative pixels; acc [F,H,W] in eighths, so that values fall on both
  sides of the threshold and on it; rgb [F,H,W,3]."""
  rs = np.random.default_rng(seed)
  depth = rs.uniform(0.5, 4., (F, H, W)).astype(np.float32)
  bad = rs.integers(0, 12, depth.shape)
  for code, value in ((0, 0.), (1, np.inf), (2, np.nan), (3, -1.5)):
    depth[bad == code] = value
  acc = (rs.integers(0, 9, depth.shape) / 8.).astype(np.float32)
  return depth, acc, rs.uniform(0., 1., (F, H, W, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, F=3, colors=True, batches=None):
  """(inputs, the restatement's volumes, its branch counts): computed once, shared, never written to.  `batches` splits the F
  frames into successive calls."""
  origin, spacing = grid_frame(shape)
  depth, acc, rgb = images(F, sum(shape) + F)
  proj = np.stack([cameras()[f % 3] for f in range(F)])
  tsdf, weight, color = T.new_volume(shape, colors)
  stats = {}
  f0 = 0
  for n in (batches or (F,)):
    sl = slice(f0, f0 + n)
    T.integrate(tsdf, weight, color, origin, spacing, TRUNC, proj[sl], depth[sl], acc=acc[sl] if colors else None,
                rgb=rgb[sl] if colors else None, acc_threshold=THRESHOLD, stats=stats)
    f0 += n
  arrays = (depth, acc, rgb, proj, tsdf, weight) + ((color,) if colors else ())
  for a in arrays:
    a.setflags(write=False)
  return dict(origin=origin, spacing=spacing, depth=depth, acc=acc, rgb=rgb, proj=proj), (tsdf, weight, color), stats


def dev(a):
  return None if a is None else torch.from_numpy(np.array(a)).cuda()


def run(shape, inp, colors=True, batches=None):
  """The kernel on the inputs of `case` -> (tsdf, weight, color) host arrays."""
  tsdf, weight, color = (dev(a) for a in T.new_volume(shape, colors))
  F = inp['depth'].shape[0]
  f0 = 0
  for n in (batches or (F,)):
    sl = slice(f0, f0 + n)
    ops.tsdf_integrate(tsdf, weight, color, inp['origin'], inp['spacing'], TRUNC, dev(inp['proj'][sl]), dev(inp['depth'][sl]),
                       acc=dev(inp['acc'][sl]) if colors else None, rgb=dev(inp['rgb'][sl]) if colors else None, acc_threshold=THRESHOLD)
    f0 += n
  return tuple(None if t is None else t.cpu().numpy() for t in (tsdf, weight, color))


def bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def assert_same_volumes(got, want):
  for name, g, w in zip(('tsdf', 'weight', 'color'), got, want):
    assert (g is None) == (w is None), name
    if g is not None:
      differ = int((bits(g) != bits(w)).sum())
      assert differ == 0, f'{name}: {differ} of {g.size} values differ, max |kernel - numpy| {np.nanmax(np.abs(g - w)):.3e}'


@pytest.mark.parametrize('colors', [True, False], ids=['acc_rgb', 'bare'])
@pytest.mark.parametrize('shape', GRIDS, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_against_the_restatement(shape, colors):
  inp, want, stats = case(shape, colors=colors)
  print(f'{shape}: {stats}')
  # every way through the seven steps is taken: behind the camera, off the image, an empty ray, no measurement, occluded
  # beyond the truncation (s < -trunc), inside it (-trunc <= s < trunc), free space in front of it (s >= trunc)
  for branch in ('behind', 'off_image', 'no_measurement', 'occluded', 'near', 'far') + (('empty',) if colors else ()):
    assert stats[branch] > 0, branch
  assert (want[1] == 0).any() and (want[1] >= 2).any()      # voxels no frame observed, voxels several did
  assert_same_volumes(run(shape, inp, colors), want)


def test_acc_values_fall_on_both_sides_of_the_threshold_and_on_it():
  acc = case(GRIDS[0])[0]['acc']
  assert (acc < THRESHOLD).any() and (acc == THRESHOLD).any() and (acc > THRESHOLD).any()


def test_batching():
  """9 frames in one call against 3 + 3 + 3: the weights are equal; tsdf and colour agree up to rounding.

  Bound.  With n <= 9 observations |t| <= 1 and 0 <= rgb <= 1 each, every numerator (a partial sum, W0 * average, their sum) is
  at most the voxel's final weight Wf in magnitude, and a quotient at most 1, i.e. Wf in numerator units; so each float32
  rounding adds at most 2^-24 Wf to the final numerator, 2^-24 to the final average.  One call makes 8 additions and a division
  (9 roundings); three calls make 2 additions, a product, an addition and a division each (15).  The two results therefore
  differ by at most 24 * 2^-24 (to first order; 1 % is added for the higher orders)."""
  shape = (9, 10, 11)
  inp, one, _ = case(shape, F=9)
  _, three, _ = case(shape, F=9, batches=(3, 3, 3))
  got_one, got_three = run(shape, inp), run(shape, inp, batches=(3, 3, 3))
  assert_same_volumes(got_one, one)
  assert_same_volumes(got_three, three)
  assert np.array_equal(got_one[1], got_three[1]) and got_one[1].max() >= 6
  bound = 24 * 2. ** -24 * 1.01
  for name, a, b in (('tsdf', got_one[0], got_three[0]), ('color', got_one[2], got_three[2])):
    err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    print(f'batching: {name} max |one call - three calls| {err:.3e} (bound {bound:.3e})')
    assert err <= bound
  assert (bits(got_one[0]) != bits(got_three[0])).any()     # (the comparison is not vacuous: the association does differ)


def test_more_frames_than_one_launch_stages():
  F = _lib.TSDF_MAX_FRAMES + 6
  assert T.MAX_FRAMES == _lib.TSDF_MAX_FRAMES
  shape = (9, 10, 11)
  inp, want, _ = case(shape, F=F)
  assert want[1].max() > _lib.TSDF_MAX_FRAMES / 3
  assert_same_volumes(run(shape, inp), want)
  # one call = a call with the first 64 frames followed by a call with the rest
  assert_same_volumes(run(shape, inp, batches=(_lib.TSDF_MAX_FRAMES, 6)), want)


def test_two_runs_agree_bit_for_bit():
  inp, _, _ = case(GRIDS[0])
  assert_same_volumes(run(GRIDS[0], inp), run(GRIDS[0], inp))


def test_wrapper_refuses_inconsistent_arguments():
  shape = (4, 4, 4)
  tsdf, weight, color = (dev(a) for a in T.new_volume(shape))
  proj, depth, rgb = dev(cameras()), torch.ones((3, H, W), device='cuda'), torch.ones((3, H, W, 3), device='cuda')
  with pytest.raises(ValueError, match='both given or both None'):
    ops.tsdf_integrate(tsdf, weight, color, (0., 0., 0.), 1., 1., proj, depth)
  with pytest.raises(ValueError, match='both given or both None'):
    ops.tsdf_integrate(tsdf, weight, None, (0., 0., 0.), 1., 1., proj, depth, rgb=rgb)
  with pytest.raises(ValueError, match=r'proj \[F,3,4\]'):
    ops.tsdf_integrate(tsdf, weight, None, (0., 0., 0.), 1., 1., proj[:2], depth)
  with pytest.raises(ValueError, match='trunc'):
    ops.tsdf_integrate(tsdf, weight, None, (0., 0., 0.), 1., 0., proj, depth)
  assert torch.equal(tsdf, torch.ones_like(tsdf)) and not weight.any()


# ---- the validity filter of ops.marching_tetrahedra


@functools.lru_cache(maxsize=None)
def filter_case(shape, seed):
  rs = np.random.default_rng(seed)
  field = rs.standard_normal(shape).astype(np.float32)
  valid = rs.random(shape) >= 0.2
  origin, spacing, level = (-0.3, 0.2, 1.), 0.37, 0.1
  full = R.marching_tetrahedra(field, level, origin, spacing)
  want = T.filter_mesh(field, level, valid, *full)
  for a in (field, valid) + full + want:
    a.setflags(write=False)
  return (field, level, origin, spacing), valid, full, want


def mt(args, **kw):
  field, level, origin, spacing = args
  return tuple(t.cpu().numpy() for t in ops.marching_tetrahedra(dev(field), level, origin, spacing, **kw))


@pytest.mark.parametrize('shape,seed', [((2, 3, 130), 11), ((9, 11, 12), 12)], ids=['2x3x130', '9x11x12'])
def test_valid_filter_against_the_restatement(shape, seed):
  args, valid, full, (rv, rn, rf, keys) = filter_case(shape, seed)
  verts, normals, faces, edges = mt(args, valid=dev(valid), return_edges=True)
  print(f'{shape}: V {len(full[0])} -> {len(rv)}, T {len(full[2])} -> {len(rf)}')
  assert 0 < len(rf) < len(full[2]) and 0 < len(rv) < len(full[0])
  assert verts.shape == rv.shape and np.array_equal(bits(verts), bits(rv))      # positions: bit for bit, order included
  assert np.abs(normals - rn).max() <= 1e-6                                     # (as tests/test_gpu_mesh.py: sqrt and division)
  assert faces.dtype == np.int32 and np.array_equal(R.canonical_faces(faces), R.canonical_faces(rf))
  assert np.array_equal(np.sort(faces, 1), np.sort(rf, 1))                      # and in the stated order
  assert np.array_equal(edges, np.stack([np.ravel_multi_index(tuple(keys[:, :3].T), shape), keys[:, 3]], -1))
  # a uint8 mask is the same mask
  again = mt(args, valid=dev(valid.astype(np.uint8)))
  assert np.array_equal(bits(again[0]), bits(verts)) and np.array_equal(again[2], faces)


def test_valid_none_and_all_valid_equal_the_unfiltered_mesh():
  args, _, full, _ = filter_case((9, 11, 12), 12)
  plain = mt(args)
  assert len(plain) == 3 and np.array_equal(bits(plain[0]), bits(full[0]))
  assert np.array_equal(R.canonical_faces(plain[2]), R.canonical_faces(full[2]))
  for out in (mt(args, valid=None), mt(args, valid=dev(np.ones(args[0].shape, bool)))):
    assert len(out) == 3
    for a, b in zip(out, plain):
      assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_all_invalid_gives_an_empty_mesh():
  args, _, _, _ = filter_case((9, 11, 12), 12)
  verts, normals, faces, edges = mt(args, valid=dev(np.zeros(args[0].shape, bool)), return_edges=True)
  assert verts.shape == (0, 3) and normals.shape == (0, 3) and faces.shape == (0, 3) and edges.shape == (0, 2)
  assert verts.dtype == np.float32 and faces.dtype == np.int32


# ---- the sphere scene, end to end through TsdfVolume


def test_sphere_scene_through_tsdf_volume():
  scene, ref = T.sphere_scene(), T.sphere_reference()
  volume = mesh.TsdfVolume(*T.SPHERE_BOX, T.SPHERE_RES, trunc_voxels=T.SPHERE_TRUNC_VOXELS)
  assert volume.shape == (33, 33, 33) and volume.spacing == T.SPHERE_SPACING and volume.trunc == 3 * T.SPHERE_SPACING
  assert torch.equal(volume.tsdf, torch.ones_like(volume.tsdf)) and not volume.weight.any() and not volume.color.any()
  volume.integrate(*(np.array(scene[k]) for k in ('depth', 'proj', 'acc', 'rgb')))
  assert_same_volumes(tuple(t.cpu().numpy() for t in (volume.tsdf, volume.weight, volume.color)), (ref['tsdf'], ref['weight'], ref['color']))
  # one frame, then a stack: the same observations, averaged in another association
  other = mesh.TsdfVolume(*T.SPHERE_BOX, T.SPHERE_RES, trunc_voxels=T.SPHERE_TRUNC_VOXELS)
  other.integrate(*(np.array(scene[k][0]) for k in ('depth', 'proj', 'acc', 'rgb')))
  other.integrate(*(np.array(scene[k][1:]) for k in ('depth', 'proj', 'acc', 'rgb')))
  assert torch.equal(other.weight, volume.weight) and (other.tsdf - volume.tsdf).abs().max() <= 1e-5
  want = ref['mesh']
  got = {k: v.cpu().numpy() for k, v in volume.mesh().items()}
  assert got['vertices'].shape == want['vertices'].shape and np.array_equal(bits(got['vertices']), bits(want['vertices']))
  assert np.array_equal(R.canonical_faces(got['faces']), R.canonical_faces(want['faces']))
  assert got['colors'].dtype == np.uint8 and np.array_equal(got['colors'], want['colors'])
  assert np.abs(got['normals'] - want['normals']).max() <= 1e-6
  stats = mesh.mesh_stats(got['vertices'], got['faces'])
  T.check_sphere_mesh(got['vertices'], got['normals'], got['faces'], stats)
  # the figures of profiles/tsdf_mesh.md
  assert (stats['V'], stats['T']) == (5282, 10560)
  unfiltered = ops.marching_tetrahedra(volume.field()[0], 0., volume.origin, volume.spacing)[2]
  assert len(unfiltered) == want['faces_unfiltered'] == 15864 and int((volume.weight == 0).sum()) == 1357


# ---- a small model (blender_256 at width 128, as tests/test_gpu_mesh.py sets it up), random weights

BINDS = ["Config.dataset_loader = 'procedural'", 'NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'NerfMLP.bottleneck_width = 128']
BOX = ((-1., -1., -1.), (1., 1., 1.))
RES, SEED, STRIDE = 17, 20200823, 16


@pytest.fixture(scope='module')
def model_case():
  from multinerf_amd import configs, datasets, models
  config = configs.load_preset('blender_256', BINDS)
  model, variables = models.construct_model(SEED, None, config, device='cuda')
  dataset = datasets.load_dataset('train', config.data_dir, config, device='cuda')
  result, volume = mesh.tsdf_mesh(model, variables, dataset, config, *BOX, RES, frame_stride=STRIDE)
  return dict(config=config, model=model, variables=variables, dataset=dataset, result=result, volume=volume)


def test_tsdf_mesh_is_the_renders_through_the_ops(model_case):
  from multinerf_amd import models, train_utils
  config, model, dataset, volume = (model_case[k] for k in ('config', 'model', 'dataset', 'volume'))
  render_fn = train_utils.create_render_fn(model)
  frames = list(range(0, dataset.size, STRIDE))
  assert len(frames) == 3 and tuple(volume.shape) == (RES,) * 3
  depth, acc, rgb, proj = [], [], [], []
  for idx in frames:
    r = models.render_image(lambda rng, rays: render_fn(model_case['variables'], 1.0, None, rays), dataset.generate_ray_batch(idx).rays,
                            None, config, verbose=False)
    depth.append(r['distance_median'].float())
    acc.append(r['acc'].float())
    rgb.append(r['rgb'].float())
    proj.append(torch.as_tensor(mesh.world_to_pixel(dataset.pixtocams, dataset.camtoworlds[idx])).cuda())
  tsdf = torch.ones((RES,) * 3, device='cuda')
  weight, color = torch.zeros_like(tsdf), torch.zeros((RES,) * 3 + (3,), device='cuda')
  ops.tsdf_integrate(tsdf, weight, color, BOX[0], volume.spacing, 3 * volume.spacing, torch.stack(proj).contiguous(),
                     torch.stack(depth).contiguous(), acc=torch.stack(acc).contiguous(), rgb=torch.stack(rgb).contiguous())
  assert torch.equal(tsdf, volume.tsdf) and torch.equal(weight, volume.weight) and torch.equal(color, volume.color)
  assert (weight > 0).any()
  field = torch.where(weight > 0, -tsdf, torch.full_like(tsdf, -1.))
  verts, normals, faces = ops.marching_tetrahedra(field, 0., BOX[0], volume.spacing, valid=weight > 0)
  result = model_case['result']
  assert torch.equal(verts, result['vertices']) and torch.equal(normals, result['normals']) and torch.equal(faces, result['faces'])
  assert result['colors'].dtype == torch.uint8 and tuple(result['colors'].shape) == tuple(verts.shape)
  print(f'model: V {len(verts)} T {len(faces)}, {int((weight == 0).sum())} of {weight.numel()} voxels never observed')
  no_colors, v2 = mesh.tsdf_mesh(model, model_case['variables'], dataset, config, *BOX, RES, frame_stride=STRIDE, colors=False)
  assert no_colors['colors'] is None and v2.color is None and torch.equal(no_colors['vertices'], verts) and torch.equal(v2.tsdf, tsdf)


def run_script(args):
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'extract_mesh.py')] + args, capture_output=True, text=True,
                     env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
  print(r.stdout[-2000:], r.stderr[-2000:])
  assert r.returncode == 0
  return r.stdout


def test_script(model_case, tmp_path):
  """extract_mesh.py --method tsdf writes mesh.tsdf_mesh's mesh, with nothing on disk but the checkpoint; without --method it
  writes mesh.extract_mesh's bytes, as before."""
  from multinerf_amd import checkpoints, train_utils
  ck = str(tmp_path / 'ckpt')
  state, _ = train_utils.create_optimizer(model_case['config'], model_case['variables'])
  state.step = 7
  checkpoints.save_checkpoint(ck, model_case['model'], state, 7)
  common = ['--preset', 'blender_256']
  for b in BINDS + [f"Config.checkpoint_dir = '{ck}'"]:
    common += ['--gin_bindings', b]
  common += ['--resolution', str(RES), '--bbox', '-1,-1,-1,1,1,1']

  out = str(tmp_path / 'tsdf.ply')
  stdout = run_script(common + ['--method', 'tsdf', '--tsdf_stride', str(STRIDE), '--out', out])
  want = str(tmp_path / 'want_tsdf.ply')
  mesh.write_ply(want, model_case['result'])
  assert open(out, 'rb').read() == open(want, 'rb').read()
  s = mesh.mesh_stats(model_case['result']['vertices'], model_case['result']['faces'])
  unseen = int((model_case['volume'].weight == 0).sum())
  assert f"mesh_stats: V {s['V']}, T {s['T']}, E {s['E']}, euler {s['euler']}" in stdout
  assert f'never observed: {unseen} of {RES ** 3} voxels' in stdout
  assert f"before the validity filter, {s['T']} after" in stdout and 'faces: ' in stdout
  assert all(w in stdout for w in ('seconds: render ', 'fusion ', 'isosurface ', 'file write '))

  threshold, chunk = 1.0, 2000
  stdout = run_script(common + ['--density_threshold', repr(threshold), '--chunk', str(chunk)])
  mesh.write_ply(want, mesh.extract_mesh(model_case['model'], *BOX, RES, threshold, chunk=chunk))
  assert open(os.path.join(ck, 'mesh', 'mesh_step_7.ply'), 'rb').read() == open(want, 'rb').read()
  assert 'seconds: grid query' in stdout and 'never observed' not in stdout
