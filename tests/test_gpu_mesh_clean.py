"""Mesh clean-up on the GPU (-m gpu): the kernels of csrc/meshclean.hip through ops.mesh_components, mesh.filter_components,
mesh.component_stats and mesh.simplify against the NumPy restatement (tests/mesh_clean_ref.py: union-find; float64 sums in the
header's order), the properties the contract promises asserted on the kernels' own output, degenerate inputs, determinism, and
extract_mesh.py with the clean-up flags.  The meshes are tests/mesh_ref.py's marching-tetrahedra meshes, a few thousand
vertices each; tests/test_mesh_clean_cpu.py holds the preconditions (known answers of the restatement, the branch margin)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import mesh_clean_ref as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_device(m):
  return {k: (None if v is None else torch.from_numpy(np.array(v)).cuda()) for k, v in m.items()}


def to_host(m):
  return {k: (None if v is None else v.cpu().numpy()) for k, v in m.items()}


def bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def labels_of(faces, n_verts):
  out = ops.mesh_components(torch.from_numpy(np.array(faces, np.int32).reshape(-1, 3)).cuda(), n_verts)
  assert out.dtype == torch.int32 and tuple(out.shape) == (n_verts,)
  return out.cpu().numpy()


def union_mesh():
  """sphere + torus + the level-1.0 noise mesh with the vertex ids permuted (seed 11), and without the permutation."""
  plain = C.concat([C.source_mesh(n)[0] for n in ('sphere', 'torus', 'noise1')])
  return C.permute_vertices(plain, 11), plain


# ---- components

@pytest.mark.parametrize('name,V,T,count,largest', [('noise', 2046, 4080, 14, [2856, 424, 396, 92, 48]), ('noise1', 1272, 2404, 35, None)])
def test_components_of_the_noise_meshes(name, V, T, count, largest):
  m, _ = C.source_mesh(name)
  assert (len(m['vertices']), len(m['faces'])) == (V, T)
  labels = labels_of(m['faces'], V)
  assert np.array_equal(labels, C.components(m['faces'], V))
  assert len(np.unique(labels)) == count
  stats = mesh.component_stats(to_device(m))
  assert stats['count'] == count and sum(stats['faces']) == T and sum(stats['vertices']) == V
  assert stats['faces'] == sorted(stats['faces'], reverse=True) and (largest is None or stats['faces'][:5] == largest)


def test_components_of_a_permuted_union():
  m, _ = union_mesh()
  labels = labels_of(m['faces'], len(m['vertices']))
  assert np.array_equal(labels, C.components(m['faces'], len(m['vertices']))) and len(np.unique(labels)) == 1 + 1 + 35


def test_a_label_travels_the_length_of_a_strip():
  faces, perm = C.strip(4096, 3)
  labels, sweeps = ops.mesh_components(torch.from_numpy(faces).cuda(), 4096, return_sweeps=True)
  print(f'strip of 4096 vertices: {sweeps} sweeps')
  assert (labels.cpu().numpy() == 0).all() and sweeps >= 2
  faces, perm = C.strip(4096, 3, drop=(2000, 2001))           # vertices 0 .. 2001 | 2002 .. 4095
  labels = labels_of(faces, 4096)
  want = np.empty((4096,), np.int32)
  want[perm[:2002]], want[perm[2002:]] = perm[:2002].min(), perm[2002:].min()
  assert np.array_equal(labels, want) and np.array_equal(labels, C.components(faces, 4096)) and len(np.unique(labels)) == 2


def test_components_edge_cases():
  assert np.array_equal(labels_of(np.zeros((0, 3), np.int32), 5), np.arange(5))
  assert labels_of(np.zeros((0, 3), np.int32), 0).shape == (0,)
  faces = np.array([[7, 2, 9], [9, 4, 2], [1, 5, 6]], np.int32)                      # 0, 3, 8 are in no face
  assert np.array_equal(labels_of(faces, 10), [0, 1, 2, 3, 2, 1, 1, 2, 8, 2])
  for bad in (-1, 10):
    with pytest.raises(ValueError):
      labels_of(np.array([[0, 1, 2], [3, bad, 4]], np.int32), 10)
  m, _ = union_mesh()
  a, b = labels_of(m['faces'], len(m['vertices'])), labels_of(m['faces'], len(m['vertices']))
  assert np.array_equal(a, b)


# ---- filter

def assert_same_mesh(got, want):
  for k in ('vertices', 'normals'):
    assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(want[k])), k
  assert got['faces'].dtype == np.int32 and np.array_equal(got['faces'], want['faces'])
  assert (got['colors'] is None) == (want['colors'] is None) and (want['colors'] is None or np.array_equal(got['colors'], want['colors']))


def test_filter_by_face_count():
  m, _ = C.source_mesh('noise')
  out = mesh.filter_components(to_device(m), min_faces=92, return_labels=True)
  assert np.array_equal(out.pop('labels').cpu().numpy(), C.components(m['faces'], len(m['vertices'])))
  got = to_host(out)
  assert_same_mesh(got, C.filter_components(m, min_faces=92))
  assert mesh.component_stats(out)['faces'] == [2856, 424, 396, 92]
  assert mesh.mesh_stats(got['vertices'], got['faces'])['boundary_edges'] == 0
  assert_same_mesh(to_host(mesh.filter_components(to_device(m))), m)                 # nothing to drop: the mesh itself
  both = to_host(mesh.filter_components(to_device(m), min_faces=400, keep_largest=5))
  assert_same_mesh(both, C.filter_components(m, min_faces=400, keep_largest=5))
  assert len(both['faces']) == 2856 + 424


def test_keep_largest_returns_the_sphere():
  _, plain = union_mesh()
  sphere, _ = C.source_mesh('sphere')
  assert_same_mesh(to_host(mesh.filter_components(to_device(plain), keep_largest=1)), sphere)
  m, _ = C.source_mesh('noise')                                                      # 48, 48: the tie goes to the smaller label
  assert_same_mesh(to_host(mesh.filter_components(to_device(m), keep_largest=5)), C.filter_components(m, keep_largest=5))


# ---- simplify

def position_tolerance(ref_vertices, cell):
  return 2. ** -22 * np.maximum(np.abs(ref_vertices.astype(np.float64)), cell)


def in_cell_slack(got_vertices, origin, cell):
  """A vertex placed at a face of its cell may land one float32 rounding of its coordinate outside, and a member's cell index
  is taken from the float32 quotient (two more roundings, of x - o and of the division): 2^-22 of the largest magnitude."""
  return 2. ** -22 * np.maximum(np.maximum(np.abs(got_vertices.astype(np.float64)), np.abs(np.asarray(origin, np.float64))), cell)


def check_output_properties(m, got, cell, origin, ref, closed):
  V2, faces = len(got['vertices']), got['faces']
  centres = ref['centres']
  rel = got['vertices'].astype(np.float64) - centres
  assert (np.abs(rel) <= cell / 2. + in_cell_slack(got['vertices'], origin, cell)).all()            # every vertex inside its cell
  # E(x) <= E(g) per cluster, for the float32 point the kernel wrote.  That point is off the float64 one by dx: the rounding to
  # float32 (2^-24 of |m + x| per coordinate) and the solve's own error (cond * 2^-53 <= (3 / 1e-3) * 1.1e-16 = 3.3e-13 of
  # |x| <= sqrt(3) cell / 2).  E is a quadratic with curvature at most tr whose gradient inside the cell is at most
  # 2 tr sqrt(3) cell (a fallback cluster sits at g, which is no stationary point), so dx moves E by at most grad dx + tr dx^2.
  # Without that term the comparison fails in float arithmetic wherever E(g) is a rounding residue: a cluster with one member has
  # g on every plane of its faces.
  dx = 2. ** -24 * np.abs(got['vertices'].astype(np.float64)).max(-1) * np.sqrt(3.) + 3.3e-13 * cell
  slack = 2. * ref['trace'] * np.sqrt(3.) * cell * dx + ref['trace'] * dx * dx
  E_x = C.cluster_errors(m['vertices'], m['faces'], ref['map'], centres, rel)
  E_g = C.cluster_errors(m['vertices'], m['faces'], ref['map'], centres, ref['g'])
  print(f'E(x) / E(g): median {np.median(E_x / np.maximum(E_g, 1e-300)):.3f}, max E(x) - E(g) {np.max(E_x - E_g):.3e}, max slack {slack.max():.3e}')
  assert (E_x <= E_g * (1. + 1e-9) + slack).all()
  assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
  from tests import mesh_ref as R
  assert len(np.unique(R.canonical_faces(faces), axis=0)) == len(faces)                 # no face twice, up to rotation
  # every vertex is referenced, except a cluster ALL of whose faces collapsed (a floater inside one cell or along a line of
  # cells: the contract still gives its cell a vertex, as it does when the whole mesh falls into one cell); none on the closed ones
  unreferenced = np.setdiff1d(np.arange(V2), faces)
  through = ref['map'][m['faces']]
  through = through[(through[:, 0] != through[:, 1]) & (through[:, 1] != through[:, 2]) & (through[:, 0] != through[:, 2])]
  assert not np.isin(unreferenced, through).any() and (len(unreferenced) == 0 or not closed)
  displacement = np.abs(got['vertices'][ref['map']].astype(np.float64) - m['vertices'].astype(np.float64))
  assert (np.linalg.norm(displacement, axis=1) < np.sqrt(3.) * cell * (1. + 1e-6)).all()           # less than the cell diagonal
  if closed:
    assert mesh.mesh_stats(got['vertices'], faces)['signed_volume'] > 0


@pytest.mark.parametrize('name,factor,explicit', C.SIMPLIFY_CASES)
def test_simplify_against_the_restatement(name, factor, explicit):
  m, cell, origin, ref = C.simplify_case(name, factor, explicit)
  out = mesh.simplify(to_device(m), cell, origin=origin, return_map=True)
  got = to_host(out)
  assert [got[k].dtype for k in ('vertices', 'normals', 'faces', 'colors', 'map')] == [np.float32, np.float32, np.int32, np.uint8, np.int32]
  assert np.array_equal(got['map'], ref['map']) and len(got['vertices']) == len(ref['vertices'])
  assert np.array_equal(got['faces'], ref['faces'])                                    # order and winding included
  assert np.array_equal(got['colors'], ref['colors'])
  assert np.array_equal(got['fallback'], ref['fallback'])
  dp = np.abs(got['vertices'].astype(np.float64) - ref['vertices'].astype(np.float64))
  dn = np.abs(got['normals'] - ref['normals']).max()
  print(f'{name} cell {factor} h: V {len(m["vertices"])} -> {len(got["vertices"])}, T {len(m["faces"])} -> {len(got["faces"])}, '
        f'{int(got["fallback"].sum())} fallbacks, positions max |kernel - numpy| {dp.max():.3e}, normals {dn:.3e}')
  assert (dp <= position_tolerance(ref['vertices'], cell)).all()
  assert dn <= 1e-6
  used_origin = m['vertices'].min(0) if origin is None else origin
  check_output_properties(m, got, cell, used_origin, ref, closed=name in ('sphere', 'torus'))
  plain = mesh.simplify(to_device(m), cell, origin=origin)
  assert sorted(plain) == ['colors', 'faces', 'normals', 'vertices'] and torch.equal(plain['vertices'], out['vertices'])


def test_simplify_without_colours_and_twice():
  m, cell, origin, ref = C.simplify_case('noise', 2., False)
  a = mesh.simplify(to_device(m), cell, return_map=True)
  b = mesh.simplify(to_device(m), cell, return_map=True)
  for k in a:
    assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
  bare = mesh.simplify(to_device(dict(m, colors=None)), cell)
  assert bare['colors'] is None and torch.equal(bare['vertices'], a['vertices']) and torch.equal(bare['faces'], a['faces'])


def test_a_planar_patch_stays_in_its_plane():
  m, h = C.planar_patch()
  for factor in (2., 3.7):
    cell = float(np.float32(factor * h))
    got = to_host(mesh.simplify(to_device(m), cell, origin=(-0.05, -0.05, 0.), return_map=True))
    ref = C.simplify(m, cell, (-0.05, -0.05, 0.))
    assert np.array_equal(got['map'], ref['map']) and np.array_equal(got['faces'], ref['faces']) and len(got['faces']) > 0
    z = np.float64(np.float32(0.3))
    assert (np.abs(got['vertices'][:, 2].astype(np.float64) - z) <= 2. ** -22 * max(z, cell)).all()
    assert (np.abs(got['vertices'].astype(np.float64) - ref['vertices']) <= position_tolerance(ref['vertices'], cell)).all()
    assert np.abs(got['normals'] - np.array([0., 0., 1.], np.float32)).max() <= 1e-6


def test_a_corner_is_kept():
  m, corner = C.corner_patch()
  out = to_host(mesh.simplify(to_device(m), 1., origin=(0., 0., 0.), return_map=True))
  assert len(out['vertices']) == 1 and len(out['faces']) == 0 and tuple(out['faces'].shape) == (0, 3) and not out['fallback'][0]
  centroid = m['vertices'].astype(np.float64).mean(0)
  d_qem, d_centroid = np.linalg.norm(out['vertices'][0] - corner), np.linalg.norm(centroid - corner)
  print(f'corner: |qem - corner| {d_qem:.4f}, |centroid - corner| {d_centroid:.4f}')
  # three orthogonal sheets of equal area: A = (tr / 3) I, so x - corner = lam / (tr / 3 + lam) (g - corner), about 1e-3 of it
  assert d_qem < d_centroid and d_qem < 0.01 * d_centroid


def test_degenerate_cells():
  for m in (C.source_mesh('noise')[0], C.planar_patch()[0]):
    cell = float(np.float32(0.5 * C.shortest_edge(m)))
    got = to_host(mesh.simplify(to_device(m), cell, return_map=True))
    V, T = len(m['vertices']), len(m['faces'])
    assert len(got['vertices']) == V and len(got['faces']) == T and np.array_equal(got['faces'], got['map'][m['faces']])
    assert np.array_equal(np.sort(got['map']), np.arange(V))
    assert (np.abs(got['vertices'][got['map']].astype(np.float64) - m['vertices']) <= position_tolerance(m['vertices'], cell)).all()
  m = C.source_mesh('torus')[0]
  got = to_host(mesh.simplify(to_device(m), 10., return_map=True))
  assert len(got['vertices']) == 1 and tuple(got['faces'].shape) == (0, 3) and (got['map'] == 0).all()
  empty = dict(vertices=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32),
               colors=np.zeros((0, 3), np.uint8))
  got = to_host(mesh.simplify(to_device(empty), 0.5))
  assert [tuple(got[k].shape) for k in ('vertices', 'normals', 'faces', 'colors')] == [(0, 3)] * 4
  got = to_host(mesh.filter_components(to_device(empty), min_faces=3))
  assert [tuple(got[k].shape) for k in ('vertices', 'normals', 'faces', 'colors')] == [(0, 3)] * 4


def test_simplify_refuses_what_it_cannot_index():
  m = dict(C.source_mesh('noise')[0])
  for cell in (0., -1., float('nan'), float('inf')):
    with pytest.raises(ValueError, match='cell'):
      mesh.simplify(to_device(m), cell)
  with pytest.raises(ValueError, match='smallest legal cell'):
    mesh.simplify(to_device(m), 1e-6)                                                   # 11 / 1e-6 > 2^21
  with pytest.raises(ValueError, match='below the origin'):
    mesh.simplify(to_device(m), 1., origin=(5., 0., 0.))
  bad = np.array(m['vertices'])
  bad[17, 1] = np.nan
  for origin in (None, (0., 0., 0.)):
    with pytest.raises(ValueError, match='not finite'):
      mesh.simplify(to_device(dict(m, vertices=bad)), 1., origin=origin)


# ---- the script (the procedural scene, model and resolution of tests/test_gpu_mesh.py::test_script_writes_the_same_mesh)

def test_script_cleans_up_the_same_mesh(tmp_path):
  from multinerf_amd import checkpoints, configs, models, train_utils
  from tests.test_gpu_mesh import BINDS, BOX, CHUNK, RES, SEED, STD
  config = configs.load_preset('blender_256', BINDS)
  model, variables = models.construct_model(SEED, None, config, device='cuda')
  field, _, spacing = mesh.density_grid(lambda x, s: model.query_density(x[None], s)[0], *BOX, RES, std=STD, chunk=CHUNK)
  threshold = float(field.median())
  full = mesh.extract_mesh(model, *BOX, RES, threshold, std=STD, chunk=CHUNK)
  want = mesh.simplify(mesh.filter_components(full, min_faces=8), 2. * spacing)
  ck = str(tmp_path / 'ckpt')
  state, _ = train_utils.create_optimizer(config, variables)
  state.step = 7
  checkpoints.save_checkpoint(ck, model, state, 7)
  args = ['--preset', 'blender_256']
  for b in BINDS + [f"Config.checkpoint_dir = '{ck}'"]:
    args += ['--gin_bindings', b]
  args += ['--resolution', str(RES), '--bbox', '-1,-1,-1,1,1,1', '--density_threshold', repr(threshold), '--std', str(STD), '--chunk', str(CHUNK),
           '--simplify', '2', '--min_component_faces', '8']
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'extract_mesh.py')] + args, capture_output=True, text=True,
                     env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
  print(r.stdout[-2000:], r.stderr[-2000:])
  assert r.returncode == 0
  back = mesh.read_ply(os.path.join(ck, 'mesh', 'mesh_step_7.ply'))
  assert 0 < len(back['vertices']) < len(full['vertices'])
  assert_same_mesh(back, to_host(want))
  before, after = mesh.mesh_stats(full['vertices'], full['faces']), mesh.mesh_stats(want['vertices'], want['faces'])
  assert f"before clean-up: mesh_stats: V {before['V']}, T {before['T']}" in r.stdout
  assert f"after clean-up: mesh_stats: V {after['V']}, T {after['T']}" in r.stdout
  assert f"components {mesh.component_stats(full)['count']}" in r.stdout and f"components {mesh.component_stats(want)['count']}" in r.stdout
  assert ', components ' in r.stdout.split('seconds:')[1] and ', simplify ' in r.stdout.split('seconds:')[1]
