"""Mesh extraction without a GPU: the NumPy restatement of csrc/mesh.hip (tests/mesh_ref.py) against analytic ground truth,
PLY files, mesh_stats, the grid arithmetic of density_grid, the argument errors of ops.marching_tetrahedra, and the lists
and documents the new kernel file has to be on."""

import math
import os

import numpy as np
import pytest
import torch

from multinerf_amd import _lib, build, mesh, ops
from tests import mesh_ref as R
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sphere():
  return R.marching_tetrahedra(R.sphere_field(), 0., R.ORIGIN, R.H)


@pytest.fixture(scope='module')
def torus():
  return R.marching_tetrahedra(R.torus_field(), 0., R.ORIGIN, R.H)


@pytest.fixture(scope='module')
def noise():
  return R.marching_tetrahedra(R.noise_field(), 0., (0., 0., 0.), 1.)


def closed_and_oriented(verts, faces, V, T, euler):
  s = mesh.mesh_stats(verts, faces)
  print(s)
  assert (s['V'], s['T'], s['euler']) == (V, T, euler)
  assert s['boundary_edges'] == 0 and s['nonmanifold_edges'] == 0 and 2 * s['E'] == 3 * s['T']
  assert R.directed_edges_once(faces)
  assert faces.min() >= 0 and faces.max() < V and len(np.unique(faces)) == V          # no vertex is left unused
  return s


def test_sphere(sphere):
  verts, normals, faces = sphere
  closed_and_oriented(verts, faces, 5184, 10364, 2)
  assert abs(3 * R.H * R.H / (8 * (0.6 - math.sqrt(3) * R.H)) - 2.98e-3) < 1e-5
  R.sphere_bounds(verts, mesh.mesh_stats(verts, faces))
  # normals: unit, toward lower field = outward; the field's gradient is radial up to the differences' O(h^2 / r^2)
  assert np.abs(np.linalg.norm(normals, axis=1) - 1).max() < 1e-6
  radial = verts / np.linalg.norm(verts, axis=1, keepdims=True)
  assert (normals * radial).sum(-1).min() > 0.99


def test_torus(torus):
  verts, _, faces = torus
  s = closed_and_oriented(verts, faces, 4848, 9696, 0)
  ratio = s['signed_volume'] / (2 * math.pi ** 2 * 0.55 * 0.2 ** 2)
  print(f'torus: volume ratio {ratio:.4f}')
  assert 0.97 <= ratio <= 1.0


def test_noise_walks_every_sign_pattern(noise):
  verts, _, faces = noise
  s = closed_and_oriented(verts, faces, 2688, 5584, -104)
  assert s['signed_volume'] > 0
  f = R.noise_field() >= 0
  seen = set()
  for perm in R.PERMS:                                   # every sign pattern of every one of the 6 tetrahedra occurs
    c = [np.zeros(3, int)]
    for axis in perm:
      c.append(c[-1] + np.eye(3, dtype=int)[axis])
    bits = sum(f[c[r][0]:f.shape[0] - 1 + c[r][0], c[r][1]:f.shape[1] - 1 + c[r][1], c[r][2]:f.shape[2] - 1 + c[r][2]].astype(int) << r
               for r in range(4))
    seen |= {(perm, int(b)) for b in np.unique(bits)}
  assert len(seen) == 6 * 16


def test_vertex_and_face_order(noise):
  """Vertices by lower-end linear index, then direction; faces by cell: what makes the mesh indexed without a hash."""
  verts, _, faces = noise
  f = R.noise_field()
  # vertex n lies on an edge leaving point floor(position) (spacing 1, origin 0): non-decreasing in the linear index
  low = np.floor(verts.astype(np.float64) + 1e-9).astype(int)
  lin = (low[:, 0] * f.shape[1] + low[:, 1]) * f.shape[2] + low[:, 2]
  assert (np.diff(lin) >= 0).all()
  # a face's vertices belong to one cell, and cells come in linear order
  cell = np.floor(verts.astype(np.float64)[faces].min(1) + 1e-9).astype(int)
  cl = (cell[:, 0] * f.shape[1] + cell[:, 1]) * f.shape[2] + cell[:, 2]
  assert (np.diff(cl) >= 0).all()


def test_special_values_give_finite_output():
  f = R.noise_field().astype(np.float32)
  f[2, 3, 4], f[5, 5, 5], f[1, 1, 1], f[3, 3, 3] = np.nan, np.inf, -np.inf, 0.0
  verts, normals, faces = R.marching_tetrahedra(f, 0., (0., 0., 0.), 1.)
  assert np.isfinite(verts).all() and np.isfinite(normals).all() and len(faces) > 0
  s = mesh.mesh_stats(verts, faces)
  assert s['boundary_edges'] == 0 and s['nonmanifold_edges'] == 0 and R.directed_edges_once(faces)
  empty = R.marching_tetrahedra(np.full((3, 4, 5), -1.), 0., (0., 0., 0.), 1.)
  assert [a.shape for a in empty] == [(0, 3), (0, 3), (0, 3)]


def test_mesh_stats_on_a_tetrahedron():
  v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
  f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)           # counter-clockwise seen from outside
  s = mesh.mesh_stats(v, f)
  assert (s['V'], s['T'], s['E'], s['euler'], s['boundary_edges'], s['nonmanifold_edges']) == (4, 4, 6, 2, 0, 0)
  assert abs(s['signed_volume'] - 1 / 6) < 1e-15 and abs(s['area'] - (1.5 + math.sqrt(3) / 2)) < 1e-15
  assert abs(mesh.mesh_stats(v, f[:, ::-1])['signed_volume'] + 1 / 6) < 1e-15
  s = mesh.mesh_stats(torch.tensor(v), torch.tensor(f[:3]))                       # one face off: its three edges are open
  assert (s['T'], s['E'], s['euler'], s['boundary_edges']) == (3, 6, 1, 3)
  s = mesh.mesh_stats(v, np.concatenate([f, [[0, 1, 2]]]))                        # an edge with three faces
  assert s['nonmanifold_edges'] == 3
  s = mesh.mesh_stats(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
  assert (s['V'], s['T'], s['E'], s['euler'], s['signed_volume'], s['area']) == (0, 0, 0, 0, 0., 0.)


@pytest.mark.parametrize('with_colors', [True, False])
def test_ply_round_trip(tmp_path, noise, with_colors):
  verts, normals, faces = noise
  colors = np.random.default_rng(1).integers(0, 256, verts.shape, dtype=np.uint8) if with_colors else None
  path = str(tmp_path / 'm.ply')
  mesh.write_ply(path, dict(vertices=torch.tensor(verts), normals=normals, faces=torch.tensor(faces), colors=colors))
  with open(path, 'rb') as fh:
    head = fh.read(1000).split(b'end_header\n')[0].decode().split('\n')
  assert head[:3] == ['ply', 'format binary_little_endian 1.0', f'element vertex {len(verts)}']
  assert 'property list uchar int vertex_indices' in head and ('property uchar red' in head) == with_colors
  assert os.path.getsize(path) == len('\n'.join(head)) + len('end_header\n') + len(verts) * (27 if with_colors else 24) + len(faces) * 13
  back = mesh.read_ply(path)
  assert back['vertices'].dtype == np.float32 and back['faces'].dtype == np.int32
  assert np.array_equal(back['vertices'].view(np.uint32), verts.view(np.uint32))
  assert np.array_equal(back['normals'].view(np.uint32), normals.view(np.uint32)) and np.array_equal(back['faces'], faces)
  if with_colors:
    assert back['colors'].dtype == np.uint8 and np.array_equal(back['colors'], colors)
  else:
    assert back['colors'] is None


def test_ply_round_trip_of_an_empty_mesh(tmp_path):
  path = str(tmp_path / 'e.ply')
  z = np.zeros((0, 3), np.float32)
  for colors in (None, np.zeros((0, 3), np.uint8)):
    mesh.write_ply(path, dict(vertices=z, normals=z, faces=np.zeros((0, 3), np.int32), colors=colors))
    back = mesh.read_ply(path)
    assert back['vertices'].shape == (0, 3) and back['normals'].shape == (0, 3) and back['faces'].shape == (0, 3)
    assert back['faces'].dtype == np.int32 and (back['colors'] is None) == (colors is None)
  with open(path, 'wb') as fh:
    fh.write(b'ply\nformat ascii 1.0\nend_header\n')
  with pytest.raises(ValueError, match='binary_little_endian'):
    mesh.read_ply(path)


def test_density_grid_shape_and_spacing():
  calls = []

  def fn(xyz, std_world):
    calls.append((xyz.shape[0], std_world))
    return xyz[:, 0] + 10 * xyz[:, 1] + 100 * xyz[:, 2]

  # non-cubic: the longest side (y, 4.0) gets 9 points, spacing 0.5; x (1.0) -> 3, z (2.2: 0.5 does not divide it) -> ceil(4.4) + 1 = 6
  field, origin, spacing = mesh.density_grid(fn, (0., -2., 1.), (1., 2., 3.2), 9, std=0.5, chunk=50, device='cpu')
  assert tuple(field.shape) == (3, 9, 6) and spacing == 0.5 and origin == (0., -2., 1.)
  assert [c[0] for c in calls] == [50, 50, 50, 12] and all(c[1] == 0.25 for c in calls)
  i, j, k = np.meshgrid(np.arange(3), np.arange(9), np.arange(6), indexing='ij')
  want = (0.5 * i) + 10 * (-2 + 0.5 * j) + 100 * (1 + 0.5 * k)
  assert np.array_equal(field.numpy(), want.astype(np.float32))
  # a resolution that does not divide the box: spacing 2 / 6 is no float32 fraction, and every side still reaches its far face
  shape, spacing = mesh.grid_shape((-1, -1, -1), (1, 1, 0), 7)
  assert shape == (7, 7, 4) and spacing == float(np.float32(2 / 6))
  assert mesh.grid_shape((0, 0, 0), (1, 1e-3, 1), 100)[0] == (100, 2, 100)           # never fewer than 2 points
  for bad in (dict(resolution=1), dict(bbox_max=(1, 1, -1)), dict(bbox_min=(0, 0, float('nan')))):
    with pytest.raises(ValueError):
      mesh.grid_shape(**{**dict(bbox_min=(-1, -1, -1), bbox_max=(1, 1, 1), resolution=8), **bad})
  with pytest.raises(ValueError, match='chunk'):
    mesh.density_grid(fn, (0, 0, 0), (1, 1, 1), 4, chunk=0, device='cpu')


def test_marching_tetrahedra_argument_errors():
  o = (0., 0., 0.)
  with pytest.raises(ValueError, match='device tensor'):
    ops.marching_tetrahedra(torch.zeros((4, 4, 4)), 0., o, 1.)
  with pytest.raises(ValueError, match='device tensor'):
    ops.marching_tetrahedra(np.zeros((4, 4, 4), np.float32), 0., o, 1.)
  # behind the device check (a meta tensor stands in for a device tensor: nothing is launched before these raise)
  ok, ops._on_device = ops._on_device, lambda t: True
  try:
    dev = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device='meta')
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (4, 4), (2, 2, 2, 2)):
      with pytest.raises(ValueError, match='every dimension >= 2'):
        ops.marching_tetrahedra(dev(*shape), 0., o, 1.)
    with pytest.raises(ValueError, match='must be torch.float32'):
      ops.marching_tetrahedra(dev(4, 4, 4, dtype=torch.float64), 0., o, 1.)
    with pytest.raises(ValueError, match='contiguous'):
      ops.marching_tetrahedra(dev(4, 4, 8)[:, :, ::2], 0., o, 1.)
    with pytest.raises(ValueError, match='contiguous'):
      ops.marching_tetrahedra(dev(4, 4, 4).permute(2, 1, 0), 0., o, 1.)
    for spacing in (0., -1., float('inf'), float('nan')):
      with pytest.raises(ValueError, match='spacing'):
        ops.marching_tetrahedra(dev(4, 4, 4), 0., o, spacing)
    for origin in ((0., 0.), (0., float('nan'), 0.)):
      with pytest.raises(ValueError, match='origin'):
        ops.marching_tetrahedra(dev(4, 4, 4), 0., origin, 1.)
  finally:
    ops._on_device = ok


def test_c_entries_validate_their_arguments():
  """Every entry returns MNR_ERR_INVALID_ARGUMENT before a launch (no GPU is touched: the checks come first)."""
  import ctypes as C
  lib = _lib.load()
  assert lib.mnr_mt_workgroups(0) == 0 and lib.mnr_mt_workgroups(256) == 1 and lib.mnr_mt_workgroups(257) == 2
  assert lib.mnr_mt_workgroups(2 ** 33 + 1) == 2 ** 25 + 1
  a = _lib.MtArgs()
  for fn in (lib.mnr_mt_classify, lib.mnr_mt_emit_vertices, lib.mnr_mt_emit_faces):
    assert fn(None, None) == _lib.MNR_ERR_INVALID_ARGUMENT
    assert fn(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT and b'field' in lib.mnr_last_error()
  buf = (C.c_float * 64)()
  a.field = a.mask = a.counts = a.offsets = a.base = a.verts = a.normals = a.faces = C.addressof(buf)
  for bad in (dict(nx=1, ny=4, nz=4, spacing=1.), dict(nx=4, ny=4, nz=4, spacing=0.), dict(nx=4, ny=4, nz=4, spacing=float('nan')),
              dict(nx=4, ny=4, nz=4, spacing=1., origin0=float('inf'))):
    a.nx, a.ny, a.nz, a.spacing, a.origin[0] = bad['nx'], bad['ny'], bad['nz'], bad['spacing'], bad.get('origin0', 0.)
    for fn in (lib.mnr_mt_classify, lib.mnr_mt_emit_vertices, lib.mnr_mt_emit_faces):
      assert fn(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT, bad
  a.nx, a.ny, a.nz, a.spacing, a.origin[0] = 4, 4, 4, 1., 0.
  a.n_verts, a.n_faces = 2 ** 31, 2 ** 31
  assert lib.mnr_mt_emit_vertices(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT and b'2^31' in lib.mnr_last_error()
  assert lib.mnr_mt_emit_faces(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT and b'2^31' in lib.mnr_last_error()
  a.n_verts, a.n_faces, a.offsets = 1, 1, None
  assert lib.mnr_mt_emit_vertices(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT
  assert lib.mnr_mt_emit_faces(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT
  a.counts = None
  assert lib.mnr_mt_classify(C.byref(a), None) == _lib.MNR_ERR_INVALID_ARGUMENT


def test_entries_lists_and_documents():
  names = _lib.header_symbols()
  for e in ('mnr_mt_workgroups', 'mnr_mt_classify', 'mnr_mt_emit_vertices', 'mnr_mt_emit_faces'):
    assert e in names and e in _lib._PROTOS and e not in _lib.F32_ABSENT
  assert 'mesh.hip' in build.SOURCES and 'mesh.hip' in build.SOURCES_F32
  for rel, attr in (('hipsim/build.py', 'SOURCES'), ('isa_report.py', 'KERNEL_FILES')):
    assert 'mesh.hip' in getattr(tool_module(rel), attr), rel
  with open(os.path.join(build.CSRC, 'mesh.hip')) as f:
    src = f.read()
  assert '#pragma clang fp contract(off)' in src and 'atomic' not in src.split('#include')[1]
  read = lambda rel: open(os.path.join(ROOT, rel)).read()
  readme = read('README.md')
  assert readme.index('### Calling an MLP on your own Gaussians') < readme.index('### Extracting a mesh') and 'scene-dependent' in readme
  assert 'mesh.hip' in read('DESIGN.md') and 'extract_mesh.py' in readme and os.path.exists(os.path.join(ROOT, 'profiles', 'mesh_extract.md'))


def test_script_command_line():
  """extract_mesh.py's flags and defaults; a --bbox value that starts with a minus sign (the default box does) is one argument."""
  import extract_mesh
  args, box = extract_mesh.parse_args([])
  assert box == [-1., -1., -1., 1., 1., 1.] and (args.resolution, args.density_threshold, args.std) == (256, 10.0, 0.5)
  assert args.chunk == mesh.DEFAULT_CHUNK and not args.no_colors and args.out is None and args.preset is None
  for argv in (['--bbox', '-1,-1,-1,1,1,1'], ['--resolution', '17', '--bbox', '-1,-1,-1,1,1,1', '--std', '0'], ['--bbox=-1,-1,-1,1,1,1']):
    assert extract_mesh.parse_args(argv)[1] == [-1., -1., -1., 1., 1., 1.], argv
  args, box = extract_mesh.parse_args(['--preset', 'blender_256', '--gin_bindings', 'A.b = 1', '--gin_bindings', 'C.d = 2', '--bbox',
                                       '-2.5,0,1e-1,3,4,5', '--density_threshold', '-0.25', '--no_colors', '--out', 'x.ply', '--chunk', '7'])
  assert box == [-2.5, 0., 0.1, 3., 4., 5.] and args.gin_bindings == ['A.b = 1', 'C.d = 2'] and args.density_threshold == -0.25
  assert args.no_colors and args.out == 'x.ply' and args.chunk == 7 and args.preset == 'blender_256'
  for bad in ('1,2,3', '-1,-1,-1,1,1,x'):
    with pytest.raises(SystemExit, match='six numbers'):
      extract_mesh.parse_args(['--bbox', bad])


def test_grid_shape_over_many_resolutions():
  """The longest side has exactly `resolution` points whatever the float32 rounding of the spacing (512 and 300 once got 513 and
  301); every side has the fewest points that reach its far face, up to that rounding."""
  boxes = (((-1, -1, -1), (1, 1, 1)), ((0, 0, 0), (1, 1, 1)), ((-1, -1, -1), (1, 1, 0)), ((0., -2., 1.), (1., 2., 3.2)),
           ((-0.3, 0.1, 0.2), (0.6, 0.4, 0.5)), ((-4, -4, -1.3), (4, 4.0000001, 2.9)))
  for res in sorted(set(range(2, 1100)) | {1024, 2048, 4096}):
    for lo, hi in boxes:
      shape, spacing = mesh.grid_shape(lo, hi, res)
      extent = [h - l for l, h in zip(lo, hi)]
      assert max(shape) == res and shape[int(np.argmax(extent))] == res, (res, lo, hi, shape)
      assert spacing == float(np.float32(max(extent) / (res - 1)))
      for n, e in zip(shape, extent):
        assert n >= 2 and (n - 1) * spacing >= e * (1 - 1e-6), (res, lo, hi, shape)          # reaches the far face
        assert n == 2 or (n - 2) * spacing < e * (1 - 1e-7), (res, lo, hi, shape)            # and with no point to spare
  for res in (256, 300, 512, 1024):
    assert mesh.grid_shape((-1, -1, -1), (1, 1, 1), res)[0] == (res,) * 3


def test_mesh_helpers_are_shared_not_copied():
  """csrc/mesh_math.h is the one finite test, normalisation, dot / cross / sub and face-index check of the six mesh files, and
  switches contraction off itself: a copy compiled with FMAs would leave its file's bit-for-bit promise."""
  import re
  read = lambda name: open(os.path.join(build.CSRC, name)).read()
  header = read('mesh_math.h')
  assert '#pragma clang fp contract(off)' in header
  assert header.index('#pragma clang fp contract(off)') < header.index('mesh_finite(float')
  for helper in ('mesh_finite(float', 'mesh_finite(double', 'mesh_normalise(float*', 'mesh_dot(', 'mesh_sub(', 'mesh_cross(', 'mesh_face_ids('):
    assert header.count(helper) >= 1, helper
  for name in ('mesh.hip', 'tsdf.hip', 'meshclean.hip', 'atlas.hip', 'raster.hip', 'meshdist.hip'):
    src = read(name)
    assert '#include "mesh_math.h"' in src and '#pragma clang fp contract(off)' in src, name
    own = re.findall(r'\b(?!mesh_)\w+_(?:finite|normalise)\s*\(', src)
    assert not own, (name, own)
    assert not re.search(r'(\w+(?:\[\w+\])*) - \1 == 0\.', src), name       # the finite test, written out

