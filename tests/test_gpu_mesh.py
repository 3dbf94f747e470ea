"""Mesh extraction on the GPU (-m gpu): the three kernels of csrc/mesh.hip through ops.marching_tetrahedra against the NumPy
restatement (tests/mesh_ref.py: float32 positions in the same order, triangles oriented geometrically), determinism,
degenerate fields, density_grid / extract_mesh on an analytic field and on a small model, and extract_mesh.py."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_field(shape, seed):
  return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# name -> (field, level, origin, spacing).  A workgroup owns 256 consecutive points: (2,3,130) = 780 and (3,2,257) = 1542 points
# end in a ragged workgroup, their workgroup and wave boundaries fall mid-row, and every cell of theirs has corners in two
# workgroups (the x neighbour is 390 / 514 points away); (2,2,2) is one cell.
FIELDS = {
    'sphere': lambda: (R.sphere_field().astype(np.float32), 0., R.ORIGIN, R.H),
    'torus': lambda: (R.torus_field().astype(np.float32), 0., R.ORIGIN, R.H),
    'noise': lambda: (R.noise_field().astype(np.float32), 0., (0., 0., 0.), 1.),
    '2x2x2': lambda: (np.array([[[1., -1.], [-2., 3.]], [[-1., 2.], [0.5, -0.25]]], np.float32), 0.125, (0.5, -1., 2.), 0.25),
    '2x3x130': lambda: (random_field((2, 3, 130), 1), 0.1, (-0.3, 0.2, 1.), 0.37),
    '3x2x257': lambda: (random_field((3, 2, 257), 2), -0.2, (1., 2., 3.), 1.5),
    '17x9x33': lambda: (random_field((17, 9, 33), 3), 0.5, (-1., -1., -1.), 2. / 32),
}


@functools.lru_cache(maxsize=None)
def case(name):
  """(inputs, the restatement's mesh): computed once, shared, never written to."""
  args = FIELDS[name]()
  ref = R.marching_tetrahedra(*args)
  for a in (args[0],) + ref:
    a.setflags(write=False)
  return args, ref


def run(field, level, origin, spacing):
  out = ops.marching_tetrahedra(torch.from_numpy(np.array(field)).cuda(), level, origin, spacing)
  assert [(t.dtype, t.dim(), t.shape[-1], t.is_contiguous()) for t in out] == \
      [(torch.float32, 2, 3, True), (torch.float32, 2, 3, True), (torch.int32, 2, 3, True)]
  return tuple(t.cpu().numpy() for t in out)


def bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('name', list(FIELDS))
def test_kernels_against_the_restatement(name):
  args, (rv, rn, rf) = case(name)
  verts, normals, faces = run(*args)
  assert verts.shape == rv.shape and faces.shape == rf.shape and len(rf) > 0
  assert np.array_equal(bits(verts), bits(rv))                                  # positions: bit for bit
  err = np.abs(normals - rn).max()
  print(f'{name}: V {len(verts)} T {len(faces)}, normals max |kernel - numpy| {err:.3e}')
  assert err <= 1e-6                                                            # sqrt and division may differ by an ulp; |n| <= 1
  assert np.array_equal(R.canonical_faces(faces), R.canonical_faces(rf))        # the oriented faces, as a set
  assert np.array_equal(np.sort(faces, 1), np.sort(rf, 1))                      # and in the stated order
  assert mesh.mesh_stats(verts, faces) == mesh.mesh_stats(rv, rf)
  if name in ('sphere', 'torus', 'noise'):
    s = mesh.mesh_stats(verts, faces)
    assert (s['V'], s['T'], s['euler']) == {'sphere': (5184, 10364, 2), 'torus': (4848, 9696, 0), 'noise': (2688, 5584, -104)}[name]
    assert s['boundary_edges'] == 0 and s['nonmanifold_edges'] == 0 and s['signed_volume'] > 0 and R.directed_edges_once(faces)


def test_two_runs_agree_bit_for_bit():
  args, _ = case('noise')
  a, b = run(*args), run(*args)
  for x, y in zip(a, b):
    assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize('value', [-1., 1.])
def test_a_field_that_never_crosses_the_level_gives_an_empty_mesh(value):
  verts, normals, faces = run(np.full((5, 6, 70), value, np.float32), 0., (0., 0., 0.), 1.)
  assert verts.shape == (0, 3) and normals.shape == (0, 3) and faces.shape == (0, 3)


def check_degenerate(field, level=0.):
  f = np.asarray(field, np.float32)
  verts, normals, faces = run(f, level, (0., 0., 0.), 1.)
  rv, rn, rf = R.marching_tetrahedra(f, level, (0., 0., 0.), 1.)
  assert len(faces) > 0 and np.isfinite(verts).all() and np.isfinite(normals).all()
  assert faces.min() >= 0 and faces.max() < len(verts)
  assert (verts >= 0).all() and (verts <= np.array(f.shape, np.float32) - 1).all()          # t in [0, 1]
  lengths = np.linalg.norm(normals.astype(np.float64), axis=1)
  assert (np.abs(lengths - 1) < 1e-6)[lengths > 0].all()
  assert np.array_equal(bits(verts), bits(rv)) and np.abs(normals - rn).max() <= 1e-6
  assert np.array_equal(R.canonical_faces(faces), R.canonical_faces(rf))
  return verts, faces


def test_entries_equal_to_the_level_are_inside():
  f = np.random.default_rng(4).integers(-1, 2, (6, 7, 45)).astype(np.float32)     # a third of the points sit on the level
  f = np.pad(f, 1, constant_values=-1.)
  verts, faces = check_degenerate(f)
  s = mesh.mesh_stats(verts, faces)
  assert s['boundary_edges'] == 0 and R.directed_edges_once(faces)
  # a point on the level is inside, so the vertex of an edge to an outside neighbour sits ON it (t = 0 or 1): grid positions occur
  assert (verts == np.round(verts)).all(-1).any()


def test_nans_are_outside_and_the_output_is_finite():
  f = R.noise_field().astype(np.float32)
  f[np.random.default_rng(5).random(f.shape) < 0.05] = np.nan
  f[4, 4, 4], f[2, 6, 3] = np.inf, -np.inf
  check_degenerate(f)


def sphere_density(xyz, std_world):
  x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
  return 0.6 - torch.sqrt(x * x + y * y + z * z)


def test_density_grid_and_mesh_of_an_analytic_sphere():
  grids = [mesh.density_grid(sphere_density, (-1., -1., -1.), (1., 1., 1.), 33, chunk=c) for c in (1000, 4097)]
  assert 33 ** 3 % 1000 and 33 ** 3 % 4097
  (field, origin, spacing), (field2, _, _) = grids
  assert tuple(field.shape) == (33, 33, 33) and origin == (-1., -1., -1.) and spacing == R.H
  assert torch.equal(field, field2)                                                          # whatever the chunks
  verts, normals, faces = ops.marching_tetrahedra(field, 0., origin, spacing)
  verts, normals, faces = (t.cpu().numpy() for t in (verts, normals, faces))
  R.sphere_bounds(verts, mesh.mesh_stats(verts, faces))
  assert mesh.mesh_stats(verts, faces)['signed_volume'] > 0 and R.directed_edges_once(faces)
  radial = verts / np.linalg.norm(verts, axis=1, keepdims=True)
  assert (normals * radial).sum(-1).min() > 0.99


# ---- a small model (blender_256 at width 128, as tests/test_gpu_scripts.py trains it), random weights

BINDS = ["Config.dataset_loader = 'procedural'", 'NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'NerfMLP.bottleneck_width = 128']
BOX = ((-1., -1., -1.), (1., 1., 1.))
RES, STD, CHUNK, SEED = 17, 0.5, 2000, 20200823


@pytest.fixture(scope='module')
def model_case():
  from multinerf_amd import configs, models
  config = configs.load_preset('blender_256', BINDS)
  model, variables = models.construct_model(SEED, None, config, device='cuda')
  density_fn = lambda x, s: model.query_density(x[None], s)[0]
  field, origin, spacing = mesh.density_grid(density_fn, *BOX, RES, std=STD, chunk=CHUNK)
  threshold = float(field.median())
  result = mesh.extract_mesh(model, *BOX, RES, threshold, std=STD, chunk=CHUNK)
  return dict(config=config, model=model, variables=variables, field=field, origin=origin, spacing=spacing, threshold=threshold,
              result=result)


def test_model_density_grid_is_the_models_query(model_case):
  model, field, origin, spacing = (model_case[k] for k in ('model', 'field', 'origin', 'spacing'))
  assert tuple(field.shape) == (RES,) * 3 and spacing == 0.125 and torch.isfinite(field).all()
  i, j, k = torch.meshgrid(*[torch.arange(RES, dtype=torch.float32, device='cuda')] * 3, indexing='ij')
  xyz = (torch.tensor(origin, device='cuda') + spacing * torch.stack([i, j, k], -1)).reshape(-1, 3)
  want = torch.cat([model.query_density(xyz[s:s + CHUNK][None], STD * spacing)[0] for s in range(0, RES ** 3, CHUNK)])
  assert torch.equal(field.reshape(-1), want)


def test_model_mesh(model_case):
  r, spacing = model_case['result'], model_case['spacing']
  verts, normals, faces, colors = (r[k].cpu().numpy() for k in ('vertices', 'normals', 'faces', 'colors'))
  V = len(verts)
  assert len(faces) >= 1 and faces.dtype == np.int32 and faces.min() >= 0 and faces.max() < V
  assert colors.dtype == np.uint8 and colors.shape == (V, 3) and normals.shape == (V, 3)
  lengths = np.linalg.norm(normals.astype(np.float64), axis=1)
  assert (np.minimum(np.abs(lengths - 1), lengths) < 1e-5).all()                             # unit or zero
  v2, n2, f2 = ops.marching_tetrahedra(model_case['field'], model_case['threshold'], model_case['origin'], spacing)
  assert torch.equal(v2, r['vertices']) and torch.equal(n2, r['normals']) and torch.equal(f2, r['faces'])
  # the surface is open only where it leaves the box: both ends of every boundary edge lie on one face of the box
  e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0), -1)
  edges, uses = np.unique(e, axis=0, return_counts=True)
  assert uses.max() <= 2
  ends = verts[edges[uses == 1]]                                                             # [B, 2, 3]
  on_face = ((ends == -1.).all(1) | (ends == 1.).all(1)).any(-1)
  print(f'model mesh: V {V} T {len(faces)}, {len(ends)} boundary edges')
  assert on_face.all()
  no_colors = mesh.extract_mesh(model_case['model'], *BOX, RES, model_case['threshold'], std=STD, chunk=CHUNK, colors=False)
  assert no_colors['colors'] is None and torch.equal(no_colors['faces'], r['faces'])


def test_script_writes_the_same_mesh(model_case, tmp_path):
  from multinerf_amd import checkpoints, train_utils
  ck = str(tmp_path / 'ckpt')
  state, _ = train_utils.create_optimizer(model_case['config'], model_case['variables'])
  state.step = 7
  checkpoints.save_checkpoint(ck, model_case['model'], state, 7)
  args = ['--preset', 'blender_256']
  for b in BINDS + [f"Config.checkpoint_dir = '{ck}'"]:
    args += ['--gin_bindings', b]
  args += ['--resolution', str(RES), '--bbox', '-1,-1,-1,1,1,1', '--density_threshold', repr(model_case['threshold']), '--std', str(STD),
           '--chunk', str(CHUNK)]
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'extract_mesh.py')] + args, capture_output=True, text=True,
                     env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
  print(r.stdout[-2000:], r.stderr[-2000:])
  assert r.returncode == 0
  back = mesh.read_ply(os.path.join(ck, 'mesh', 'mesh_step_7.ply'))
  want = model_case['result']
  for k in ('vertices', 'normals'):
    assert np.array_equal(bits(back[k]), bits(want[k].cpu().numpy())), k
  assert np.array_equal(back['faces'], want['faces'].cpu().numpy()) and np.array_equal(back['colors'], want['colors'].cpu().numpy())
  s = mesh.mesh_stats(want['vertices'], want['faces'])
  assert f"mesh_stats: V {s['V']}, T {s['T']}, E {s['E']}, euler {s['euler']}" in r.stdout and 'seconds: grid query' in r.stdout
