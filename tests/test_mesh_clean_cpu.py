"""Mesh clean-up without a GPU: known answers that pin the NumPy restatement (tests/mesh_clean_ref.py) the GPU tests compare the
kernels against, the precondition of those comparisons (no solve within 1e-6 cell of the boundary at which kernel and restatement
could take different branches), the C entries' argument checks, and the plumbing."""

import ctypes as C
import os

import numpy as np
import pytest

from multinerf_amd import _lib, build
from tests import mesh_clean_ref as M
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TETRA = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.int32)


def test_two_disjoint_tetrahedra_are_two_components():
  faces = np.concatenate([TETRA + 4, TETRA])                                   # ids 4..7 first, then 0..3
  assert np.array_equal(M.components(faces, 8), [0, 0, 0, 0, 4, 4, 4, 4])
  perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
  labels = M.components(perm[faces], 8)
  assert np.array_equal(labels[perm], [0, 0, 0, 0, 1, 1, 1, 1])                 # {5,2,7,0} -> 0, {3,6,1,4} -> 1
  assert np.array_equal(M.components(faces, 10)[8:], [8, 9])                    # vertices in no face
  m = dict(vertices=np.arange(24, dtype=np.float32).reshape(8, 3), normals=np.zeros((8, 3), np.float32), faces=faces[:7], colors=None)
  out = M.filter_components(m, min_faces=4)                                    # the second tetrahedron lost a face
  assert np.array_equal(out['faces'], TETRA) and np.array_equal(out['vertices'], m['vertices'][4:])
  assert np.array_equal(M.filter_components(m, keep_largest=1)['faces'], TETRA)


def test_strip_helper():
  faces, perm = M.strip(64, 3)
  assert faces.shape == (62, 3) and (M.components(faces, 64) == 0).all()
  faces, perm = M.strip(64, 3, drop=(20, 21))
  assert len(np.unique(M.components(faces, 64))) == 2


def test_noise_mesh_counts():
  for name, V, T, count in (('noise', 2046, 4080, 14), ('noise1', 1272, 2404, 35)):
    m, _ = M.source_mesh(name)
    labels = M.components(m['faces'], len(m['vertices']))
    assert (len(m['vertices']), len(m['faces']), len(np.unique(labels))) == (V, T, count)
  m, _ = M.source_mesh('noise')
  counts = sorted(M.component_face_counts(m['faces'], M.components(m['faces'], 2046)).values(), reverse=True)
  assert counts[:6] == [2856, 424, 396, 92, 48, 48]


def test_a_planar_patch_clusters_to_points_in_the_plane():
  m, h = M.planar_patch()
  for factor in (2., 3.7):
    ref = M.simplify(m, np.float32(factor * h), (-0.05, -0.05, 0.))
    assert 1 < len(ref['vertices']) < len(m['vertices']) and len(ref['faces']) > 0
    assert (np.abs(ref['vertices'][:, 2].astype(np.float64) - np.float64(np.float32(0.3))) <= 2. ** -22 * 0.3).all()
    assert np.array_equal(ref['normals'], np.tile(np.array([[0., 0., 1.]], np.float32), (len(ref['vertices']), 1)))
    # flat: A has rank 1, the regulariser decides the in-plane position, which is the centroid's
    assert np.abs(ref['x'] - ref['g'])[~ref['fallback']].max() <= 1e-9 * factor * h


def test_a_corner_is_kept():
  m, corner = M.corner_patch()
  ref = M.simplify(m, 1., (0., 0., 0.))
  assert len(ref['vertices']) == 1 and ref['faces'].shape == (0, 3) and not ref['fallback'][0]
  centroid = m['vertices'].astype(np.float64).mean(0)
  d_qem, d_centroid = np.linalg.norm(ref['vertices'][0] - corner), np.linalg.norm(centroid - corner)
  assert d_qem < d_centroid and d_qem < 0.01 * d_centroid
  assert M.quadric_error(m['vertices'], m['faces'], ref['map'], 0, ref['centres'][0], corner - ref['centres'][0]) < 1e-12
  assert M.quadric_error(m['vertices'], m['faces'], ref['map'], 0, ref['centres'][0], ref['g'][0]) > 1e-3


def test_the_solve_never_has_a_larger_error_than_the_centroid():
  """E(x) <= E(g) in float64, up to the rounding of the solve: x is exact to cond * 2^-53 <= 3.3e-13 of |x| <= sqrt(3) cell / 2, E's
  gradient inside the cell is at most 2 tr sqrt(3) cell and its curvature at most tr.  (A cluster with one member has g on
  every plane of its faces, E(g) a rounding residue: a purely relative bound cannot hold there.)"""
  for case in M.SIMPLIFY_CASES:
    m, cell, origin, ref = M.simplify_case(*case)
    x = np.where(ref['fallback'][:, None], ref['g'], ref['x'])
    E_x = M.cluster_errors(m['vertices'], m['faces'], ref['map'], ref['centres'], x)
    E_g = M.cluster_errors(m['vertices'], m['faces'], ref['map'], ref['centres'], ref['g'])
    dx = 3.3e-13 * cell
    assert (E_x <= E_g * (1. + 1e-9) + 2. * ref['trace'] * np.sqrt(3.) * cell * dx + ref['trace'] * dx * dx).all(), case
    taken = ~ref['fallback']
    assert taken.sum() > 0.8 * len(taken) and np.median(E_x[taken] / np.maximum(E_g[taken], 1e-300)) < 0.95
    k = int(np.argmax(E_g))                                                     # the two evaluations of E agree
    single = M.quadric_error(m['vertices'], m['faces'], ref['map'], k, ref['centres'][k], ref['g'][k])
    assert abs(single - E_g[k]) <= 1e-12 * E_g[k]


def test_no_solve_is_near_the_branch_of_any_case_the_gpu_tests_use():
  """The precondition of the GPU comparison: over every (mesh, cell, origin) of tests/test_gpu_mesh_clean.py no solved point,
  accepted or rejected, lies within 1e-6 cell of |x_a| = cell / 2, so kernel and restatement cannot take different branches.
  No cluster is excluded."""
  for case in M.SIMPLIFY_CASES:
    m, cell, origin, ref = M.simplify_case(*case)
    margin = M.boundary_margin(ref, cell)
    print(case, f'margin {margin:.3e} cell, {int(ref["fallback"].sum())} of {len(ref["fallback"])} clusters fall back')
    assert margin > 1e-6, case
  m, h = M.planar_patch()
  for factor in (2., 3.7):
    cell = np.float32(factor * h)
    assert M.boundary_margin(M.simplify(m, cell, (-0.05, -0.05, 0.)), cell) > 1e-6


def test_half_the_shortest_edge_separates_every_vertex():
  for m in (M.source_mesh('noise')[0], M.planar_patch()[0]):
    cell = np.float32(0.5 * M.shortest_edge(m))
    ref = M.simplify(m, cell)
    assert len(ref['vertices']) == len(m['vertices']) and np.array_equal(ref['faces'], ref['map'][m['faces']])


def test_faces_of_the_restatement():
  """Re-indexing, the distinctness rule, duplicates up to rotation (the first stays), opposite windings (both stay)."""
  verts = np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [0.2, 0.2, 0.1], [1.2, 0.2, 0.2], [0.2, 1.2, 0.2]], np.float32)
  faces = np.array([[0, 1, 2], [4, 5, 3], [0, 3, 1], [5, 4, 3], [2, 0, 1]], np.int32)
  m = dict(vertices=verts, normals=np.tile(np.array([[0., 0., 1.]], np.float32), (6, 1)), faces=faces,
           colors=np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 3, 255], [2, 1, 1], [5, 2, 2]], np.uint8))
  ref = M.simplify(m, 1., (0., 0., 0.))
  assert np.array_equal(ref['map'], [0, 2, 1, 0, 2, 1])                          # cells (0,0,0), (0,1,0), (1,0,0)
  assert np.array_equal(ref['faces'], [[0, 2, 1], [1, 2, 0]])                    # (2,1,0) repeats face 0; face 3 is its reverse
  assert np.array_equal(ref['colors'], [[1, 2, 128], [4, 2, 2], [2, 1, 1]])      # halves round up: (0 + 1) / 2 -> 1, 255 / 2 -> 128


def test_entries_check_their_arguments():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  lib, bad = _lib.load(), _lib.MNR_ERR_INVALID_ARGUMENT
  buf = (C.c_int64 * 64)()
  p = C.addressof(buf)
  assert lib.mnr_mesh_cc_init(-1, p, None) == bad and lib.mnr_mesh_cc_init(2 ** 31, p, None) == bad and b'2^31' in lib.mnr_last_error()
  assert lib.mnr_mesh_cc_init(3, None, None) == bad and lib.mnr_mesh_cc_init(0, None, None) == _lib.MNR_OK
  assert lib.mnr_mesh_cc_sweep(None, 2, 3, p, p, None) == bad and b'faces' in lib.mnr_last_error()
  assert lib.mnr_mesh_cc_sweep(p, 2, 3, p, None, None) == bad
  assert lib.mnr_mesh_cc_sweep(None, 0, 3, None, None, None) == _lib.MNR_OK and lib.mnr_mesh_cc_sweep(None, 5, 0, None, None, None) == _lib.MNR_OK
  o = (C.c_float * 3)(0., 0., 0.)
  assert lib.mnr_mesh_cluster_keys(p, 3, None, 1., p, None) == bad and b'origin' in lib.mnr_last_error()
  for cell in (0., -1., float('nan'), float('inf')):
    assert lib.mnr_mesh_cluster_keys(p, 3, o, cell, p, None) == bad and b'cell' in lib.mnr_last_error()
  assert lib.mnr_mesh_cluster_keys(p, 3, (C.c_float * 3)(0., float('inf'), 0.), 1., p, None) == bad
  assert lib.mnr_mesh_cluster_keys(None, 3, o, 1., p, None) == bad and lib.mnr_mesh_cluster_keys(None, 0, o, 1., None, None) == _lib.MNR_OK
  assert lib.mnr_mesh_cluster_faces(p, 2, p, 3, 4, p, p, p, p, None) == bad and b'clusters' in lib.mnr_last_error()
  assert lib.mnr_mesh_cluster_faces(p, 2, p, 3, 3, p, p, None, p, None) == bad
  assert lib.mnr_mesh_cluster_faces(None, 0, None, 3, 3, None, None, None, None, None) == _lib.MNR_OK
  a = _lib.MeshClusterArgs()
  assert lib.mnr_mesh_cluster_solve(None, None) == bad
  a.n_clusters, a.n_verts, a.n_faces, a.n_incident, a.cell = 2, 1, 0, 0, 1.
  assert lib.mnr_mesh_cluster_solve(C.byref(a), None) == bad and b'clusters' in lib.mnr_last_error()
  a.n_clusters, a.n_incident = 1, 1
  assert lib.mnr_mesh_cluster_solve(C.byref(a), None) == bad and b'face list' in lib.mnr_last_error()
  a.n_incident, a.cell = 0, 0.
  assert lib.mnr_mesh_cluster_solve(C.byref(a), None) == bad and b'cell' in lib.mnr_last_error()
  a.cell, a.colors = 1., p
  assert lib.mnr_mesh_cluster_solve(C.byref(a), None) == bad and b'colors' in lib.mnr_last_error()
  a.colors = None
  assert lib.mnr_mesh_cluster_solve(C.byref(a), None) == bad and b'needs' in lib.mnr_last_error()
  a.n_clusters = 0
  assert lib.mnr_mesh_cluster_solve(C.byref(a), None) == _lib.MNR_OK


ENTRIES = ('mnr_mesh_cc_init', 'mnr_mesh_cc_sweep', 'mnr_mesh_cluster_keys', 'mnr_mesh_cluster_faces', 'mnr_mesh_cluster_solve')


def test_entries_lists_and_documents():
  names = _lib.header_symbols()
  for e in ENTRIES:
    assert e in names and e in _lib._PROTOS and e not in _lib.F32_ABSENT
  header = open(_lib.HEADER_PATH).read()
  assert f'#define MNR_QEM_REG {_lib.QEM_REG:g}\n'.replace('0.001', '1e-3') in header
  assert f'#define MNR_MESH_CELL_LIMIT (1 << 21)\n' in header and _lib.MESH_CELL_LIMIT == 1 << 21 == M.CELL_LIMIT and _lib.QEM_REG == M.QEM_REG
  assert f'#define MNR_MESH_KEY_NONFINITE ({_lib.MESH_KEY_NONFINITE})' in header and f'#define MNR_MESH_KEY_OUTSIDE ({_lib.MESH_KEY_OUTSIDE})' in header
  assert 'meshclean.hip' in build.SOURCES and 'meshclean.hip' in build.SOURCES_F32
  read = lambda rel: open(os.path.join(ROOT, rel)).read()
  for rel, attr in (('hipsim/build.py', 'SOURCES'), ('isa_report.py', 'KERNEL_FILES')):
    assert 'meshclean.hip' in getattr(tool_module(rel), attr), rel
  code = read('multinerf_amd/csrc/meshclean.hip').split('#include')[1]
  assert '#pragma clang fp contract(off)' in code and 'atomicAdd' not in code and 'asm' not in code and 'float' in code
  cc = code[:code.index('// ---- vertex clustering: keys')]
  assert 'atomicMin' in cc and 'float' not in cc and 'double' not in cc           # the labelling: integers only
  readme = read('README.md')
  assert 'No simplification, component filtering or texture atlas' not in readme and '--simplify' in readme
  assert 'meshclean.hip' in read('DESIGN.md') and os.path.exists(os.path.join(ROOT, 'profiles', 'mesh_clean.md'))


def test_script_command_line():
  import extract_mesh
  args, _ = extract_mesh.parse_args([])
  assert (args.min_component_faces, args.keep_largest, args.simplify) == (0, 0, 0.)
  args, _ = extract_mesh.parse_args(['--min_component_faces', '8', '--keep_largest', '3', '--simplify', '2.5', '--method', 'tsdf'])
  assert (args.min_component_faces, args.keep_largest, args.simplify, args.method) == (8, 3, 2.5, 'tsdf')
  for bad in (['--simplify', '-1'], ['--keep_largest', '-2'], ['--min_component_faces', '-1'], ['--simplify', 'nan']):
    with pytest.raises(SystemExit):
      extract_mesh.parse_args(bad)
  assert extract_mesh._clean_up_seconds(args, 1., 2.) == ', components 1.000, simplify 2.000'
  assert extract_mesh._clean_up_seconds(extract_mesh.parse_args([])[0], 0., 0.) == ''
