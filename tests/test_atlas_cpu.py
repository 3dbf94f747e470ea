"""Texture atlas, without a GPU: known answers of the NumPy restatement (tests/atlas_ref.py) of include/mnerf.h's contract (one face
written out by hand, ownership, the UV kernel's table as the inverse of the sample map), ops.atlas_layout, the agreement of header,
prototypes and build lists, extract_mesh.py's flags, and the PLY / OBJ writers."""

import os

import numpy as np
import pytest

from multinerf_amd import _lib, build, mesh, ops
from tests import atlas_ref as A
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('mnr_atlas_samples', 'mnr_atlas_store', 'mnr_atlas_uvs')


def one_face():
  return dict(vertices=np.array([[0., 0., 0.], [1., 0., 0.], [0., 2., 0.]], np.float32),
              normals=np.array([[0., 0., 1.]] * 3, np.float32), faces=np.array([[0, 1, 2]], np.int32))


def test_one_face_at_cell_3_by_hand():
  """c = 3: a cell of 4 x 3 texels, b = x' / 1.  Lower face: X + Y <= 2."""
  s = A.samples(one_face(), 3)
  face = s['face'].reshape(3, 4)
  assert np.array_equal(face, [[0, 0, 0, -1], [0, 0, -1, -1], [0, -1, -1, -1]])        # T = 1: the upper half is invalid
  means = s['means'].reshape(3, 4, 3)
  # p = v0 + x' (v1 - v0) + y' (v2 - v0) = (x', 2 y', 0)
  for Y in range(3):
    for X in range(3 - Y):
      assert np.array_equal(means[Y, X], [X, 2 * Y, 0]), (X, Y)
  assert (means[face < 0] == 0).all() and (s['covs'].reshape(3, 4, 3, 3)[face < 0] == 0).all()
  assert np.array_equal(s['normals'].reshape(3, 4, 3)[0, 0], [0, 0, 1]) and np.array_equal(s['viewdirs'].reshape(3, 4, 3)[0, 0], [0, 0, -1])
  assert np.array_equal(s['viewdirs'].reshape(3, 4, 3)[2, 3], [0, 0, 1])              # invalid: (0, 0, 1)
  # a = (1, 0, 0), b = (0, 2, 0): cov = (1 / 12) diag(1, 4, 0)
  want = np.float32(1. / 12.) * np.diag([1., 4., 0.]).astype(np.float32)
  assert np.array_equal(s['covs'].reshape(3, 4, 3, 3)[1, 1], want)
  assert (A.samples(one_face(), 3, filter=0.)['covs'] == 0).all()
  lay = A.layout(1, 3)
  assert lay == dict(cell=3, cols=1, rows=1, W=4, H=3, n_samples=12)
  uv = A.uvs(1, lay)
  assert np.array_equal(uv[0], np.array([[.5 / 4, 1 - .5 / 3], [1.5 / 4, 1 - .5 / 3], [.5 / 4, 1 - 1.5 / 3]], np.float32))


def test_two_faces_at_cell_4_by_hand():
  """c = 4: a cell of 5 x 4 texels, b = x' / 2.  Upper face: x' = 4 - X, y' = 3 - Y."""
  m = one_face()
  m['faces'] = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
  s = A.samples(m, 4)
  face = s['face'].reshape(4, 5)
  assert np.array_equal(face, [[0, 0, 0, 0, 1], [0, 0, 0, 1, 1], [0, 0, 1, 1, 1], [0, 1, 1, 1, 1]])
  means = s['means'].reshape(4, 5, 3)
  assert np.array_equal(means[0, 2], [1, 0, 0]) and np.array_equal(means[2, 0], [0, 2, 0]) and np.array_equal(means[1, 1], [.5, 1, 0])
  assert np.array_equal(means[0, 3], [1.5, 0, 0]) and np.array_equal(means[3, 0], [0, 3, 0])       # the gutter: b0 = -1/2
  # the upper face (2, 1, 0): v0 = (0, 2, 0) at X = 4, Y = 3; v1 = (1, 0, 0) at X = 2, Y = 3; v2 = (0, 0, 0) at X = 4, Y = 1
  assert np.array_equal(means[3, 4], [0, 2, 0]) and np.array_equal(means[3, 2], [1, 0, 0]) and np.array_equal(means[1, 4], [0, 0, 0])
  assert np.array_equal(s['normals'].reshape(4, 5, 3)[3, 4], [0, 0, 1])              # the vertex normals, not the flipped winding
  uv = A.uvs(2, A.layout(2, 4))
  assert np.allclose(uv[0] * [5, 4], np.array([[.5, 4 - .5], [2.5, 4 - .5], [.5, 4 - 2.5]]), atol=1e-6, rtol=0)
  assert np.allclose(uv[1] * [5, 4], np.array([[4.5, 4 - 3.5], [2.5, 4 - 3.5], [4.5, 4 - 1.5]]), atol=1e-6, rtol=0)


@pytest.mark.parametrize('c', range(3, 10))
def test_every_texel_has_exactly_one_owner(c):
  owners = np.zeros((c, c + 1, 2), np.int64)
  for half, xl, yl, X, Y in A.local_texels(c):
    assert 0 <= X <= c and 0 <= Y <= c - 1 and xl >= 0 and yl >= 0 and xl + yl <= c - 1
    assert (half == 0) == (X + Y <= c - 1)
    owners[Y, X, half] += 1
  assert (owners.sum(-1) == 1).all() and owners[..., 0].sum() == owners[..., 1].sum() == c * (c + 1) // 2
  rng = np.random.default_rng(c)
  m = dict(vertices=rng.uniform(-1, 1, (9, 3)).astype(np.float32), normals=rng.normal(size=(9, 3)).astype(np.float32),
           faces=rng.integers(0, 9, (6, 3)).astype(np.int32))
  face = A.samples(m, c)['face'].reshape(3, c, c + 1)
  for k in range(3):
    assert set(np.unique(face[k])) == {2 * k, 2 * k + 1}


@pytest.mark.parametrize('c,cols', [(3, None), (4, 2), (5, 1), (8, None), (9, 3)])
def test_uvs_invert_samples(c, cols):
  """The UV of barycentric (1,0,0), (0,1,0), (0,0,1) is the centre of the texel whose sample is that corner of the face."""
  rng = np.random.default_rng(100 * c)
  T = 7
  m = dict(vertices=rng.uniform(-1, 1, (3 * T, 3)).astype(np.float32), normals=rng.normal(size=(3 * T, 3)).astype(np.float32),
           faces=np.arange(3 * T, dtype=np.int32).reshape(T, 3))
  lay = A.layout(T, c, cols)
  s, uv = A.samples(m, c), A.uvs(T, lay)
  per_cell = c * (c + 1)
  for f in range(T):
    for corner in range(3):
      px, py = np.float64(uv[f, corner, 0]) * lay['W'], (1. - np.float64(uv[f, corner, 1])) * lay['H']
      X, Y = int(np.floor(px)), int(np.floor(py))
      assert abs(px - (X + .5)) <= 2. ** -22 * lay['W'] and abs(py - (Y + .5)) <= 2. ** -22 * lay['H']        # a texel centre, to float32
      k = (Y // c) * lay['cols'] + X // (c + 1)
      idx = k * per_cell + (Y % c) * (c + 1) + X % (c + 1)
      assert s['face'][idx] == f
      assert np.array_equal(s['means'][idx], m['vertices'][m['faces'][f, corner]]), (f, corner)


def test_atlas_layout():
  for c in (3, 4, 8, 13):
    for T in (0, 1, 2, 3, 101):
      ncells = (T + 1) // 2
      for cols in (None, 1):
        lay = ops.atlas_layout(T, c, cols)
        assert lay == A.layout(T, c, cols), (c, T, cols)
        assert lay['n_samples'] == ncells * c * (c + 1) and lay['cell'] == c and lay['cols'] >= 1
        if T == 0:
          assert (lay['rows'], lay['W'], lay['H']) == (0, 0, 0)
          continue
        assert lay['W'] == lay['cols'] * (c + 1) and lay['H'] == lay['rows'] * c and lay['rows'] == -(-ncells // lay['cols'])
        assert lay['W'] * lay['H'] >= lay['n_samples'] > lay['W'] * (lay['H'] - c)
        if cols == 1:
          assert (lay['cols'], lay['rows']) == (1, ncells)
        else:                                                 # the smallest cols with cols^2 (c + 1) >= ncells c: roughly square
          assert lay['cols'] ** 2 * (c + 1) >= ncells * c and (lay['cols'] == 1 or (lay['cols'] - 1) ** 2 * (c + 1) < ncells * c)
  assert ops.atlas_layout(101, 8) == dict(cell=8, cols=7, rows=8, W=63, H=64, n_samples=51 * 72)
  assert ops.atlas_layout(2_000_000, 8)['cols'] == 943                              # ceil(sqrt(1e6 * 8 / 9))
  for bad in (dict(cell=2), dict(cell=0), dict(cell=3, cols=0), dict(cell=3, n_faces=-1)):
    with pytest.raises(ValueError):
      ops.atlas_layout(bad.get('n_faces', 4), bad['cell'], bad.get('cols'))


def test_entries_lists_and_documents():
  names = _lib.header_symbols()
  for e in ENTRIES:
    assert e in names and e in _lib._PROTOS and e not in _lib.F32_ABSENT
  read = lambda rel: open(os.path.join(ROOT, rel)).read()
  header = read('include/mnerf.h')
  assert f'#define MNR_ATLAS_MIN_CELL {_lib.ATLAS_MIN_CELL}\n' in header and _lib.ATLAS_MIN_CELL == 3 == A.MIN_CELL
  assert 'seam-safe' in header and 'is exactly 0' in header and 'GUTTER' in header
  assert 'atlas.hip' in build.SOURCES and 'atlas.hip' in build.SOURCES_F32
  for rel, attr in (('hipsim/build.py', 'SOURCES'), ('isa_report.py', 'KERNEL_FILES')):
    assert 'atlas.hip' in getattr(tool_module(rel), attr), rel
  code = read('multinerf_amd/csrc/atlas.hip').split('#include')[1]
  assert '#pragma clang fp contract(off)' in code and 'atomic' not in code and 'asm' not in code
  assert code.count('atlas_chart_of(') >= 3 and '__host__ __device__' in code      # one helper, the sample and the UV kernel use it
  fields = dict(_lib.AtlasArgs._fields_)
  assert list(fields) == ['verts', 'normals', 'faces', 'n_verts', 'n_faces', 'c', 'cols', 'W', 'H', 'cov_scale']
  readme = read('README.md')
  assert 'there is still no texture atlas' not in readme and '--texture' in readme and 'bake_texture' in readme
  assert 'atlas.hip' in read('DESIGN.md') and os.path.exists(os.path.join(ROOT, 'profiles', 'texture_atlas.md'))
  assert os.path.exists(os.path.join(ROOT, 'tools', 'atlas_probe.py'))


def test_script_command_line():
  import extract_mesh
  args, _ = extract_mesh.parse_args([])
  assert (args.texture, args.texture_filter, args.texture_max_side) == (0, 1.0, 16384)
  args, _ = extract_mesh.parse_args(['--texture', '8', '--texture_filter', '0', '--texture_max_side', '4096', '--out', 'x.obj', '--method', 'tsdf'])
  assert (args.texture, args.texture_filter, args.texture_max_side, args.out, args.method) == (8, 0., 4096, 'x.obj', 'tsdf')
  assert extract_mesh.parse_args(['--texture', '3'])[0].texture == 3
  for bad in (['--texture', '2'], ['--texture', '-1'], ['--texture_filter', 'nan'], ['--texture_filter', '-1'], ['--texture_filter', 'inf'],
              ['--texture_max_side', '0']):
    with pytest.raises(SystemExit):
      extract_mesh.parse_args(bad)
  assert extract_mesh._texture_seconds(args, 1.5) == ', texture bake 1.500' and extract_mesh._texture_seconds(extract_mesh.parse_args([])[0], 0.) == ''


# ---- files

def small_mesh(colors=True):
  rng = np.random.default_rng(5)
  V, T = 7, 5
  m = dict(vertices=rng.uniform(-1, 1, (V, 3)).astype(np.float32), normals=rng.normal(size=(V, 3)).astype(np.float32),
           faces=rng.integers(0, V, (T, 3)).astype(np.int32), colors=rng.integers(0, 256, (V, 3)).astype(np.uint8) if colors else None)
  lay = A.layout(T, 4)
  tex = dict(texture=rng.integers(0, 256, (lay['H'], lay['W'], 3)).astype(np.uint8), uv=A.uvs(T, lay), layout=lay)
  return m, tex


def parent_ply_bytes(m):
  """The file the writer wrote before it knew textures, built here from the layout it documents."""
  V, T, colors = len(m['vertices']), len(m['faces']), m['colors']
  header = ['ply', 'format binary_little_endian 1.0', f'element vertex {V}'] + [f'property float {n}' for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')]
  header += [f'property uchar {n}' for n in ('red', 'green', 'blue')] if colors is not None else []
  header += [f'element face {T}', 'property list uchar int vertex_indices', 'end_header']
  body = b''
  for i in range(V):
    body += m['vertices'][i].astype('<f4').tobytes() + m['normals'][i].astype('<f4').tobytes()
    body += colors[i].tobytes() if colors is not None else b''
  for t in range(T):
    body += b'\x03' + m['faces'][t].astype('<i4').tobytes()
  return ('\n'.join(header) + '\n').encode('ascii') + body


@pytest.mark.parametrize('colors', [True, False])
def test_ply_without_a_texture_is_the_file_written_before(tmp_path, colors):
  m, _ = small_mesh(colors)
  path = str(tmp_path / 'plain.ply')
  mesh.write_ply(path, m)
  assert open(path, 'rb').read() == parent_ply_bytes(m)
  mesh.write_ply(path, m, texture=None)
  assert open(path, 'rb').read() == parent_ply_bytes(m) and os.listdir(tmp_path) == ['plain.ply']
  back = mesh.read_ply(path)
  assert sorted(back) == ['colors', 'faces', 'normals', 'vertices']


def test_ply_round_trip_with_texcoord(tmp_path):
  from PIL import Image
  m, tex = small_mesh()
  path = str(tmp_path / 'scene.v2.ply')
  mesh.write_ply(path, m, texture=tex)
  assert sorted(os.listdir(tmp_path)) == ['scene.v2.ply', 'scene.v2.png']
  head = open(path, 'rb').read().split(b'end_header\n')[0].decode('ascii').split('\n')
  assert head[2] == 'comment TextureFile scene.v2.png' and head[-2:] == ['property list uchar float texcoord', '']
  back = mesh.read_ply(path)
  assert back['texture_file'] == 'scene.v2.png' and back['texcoord'].dtype == np.float32
  assert np.array_equal(back['texcoord'].view(np.uint32), tex['uv'].view(np.uint32))
  for k in ('vertices', 'normals', 'faces', 'colors'):
    assert np.array_equal(back[k], m[k]), k
  assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'scene.v2.png'))), tex['texture'])
  with pytest.raises(ValueError):
    mesh.write_ply(path, m, texture=dict(tex, uv=tex['uv'][:-1]))
  with pytest.raises(ValueError):
    mesh.write_ply(path, m, texture=dict(tex, texture=np.zeros((0, 0, 3), np.uint8)))


def test_obj(tmp_path):
  from PIL import Image
  m, tex = small_mesh()
  V, T = len(m['vertices']), len(m['faces'])
  path = str(tmp_path / 'scene.obj')
  mesh.write_obj(path, m, tex)
  assert sorted(os.listdir(tmp_path)) == ['scene.mtl', 'scene.obj', 'scene.png']
  lines = open(path).read().split('\n')
  kinds = [l.split(' ')[0] for l in lines if l]
  assert (kinds.count('v'), kinds.count('vn'), kinds.count('vt'), kinds.count('f')) == (V, V, 3 * T, T)
  assert lines[0] == 'mtllib scene.mtl' and kinds.count('usemtl') == 1 and kinds.index('usemtl') < kinds.index('f')
  num = lambda kind: np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith(kind + ' ')])
  assert np.array_equal(num('v').astype(np.float32), m['vertices']) and np.array_equal(num('vn').astype(np.float32), m['normals'])
  assert np.array_equal(num('vt').astype(np.float32), tex['uv'].reshape(-1, 2))
  f = np.array([[[int(x) for x in w.split('/')] for w in l.split()[1:]] for l in lines if l.startswith('f ')])
  assert f.shape == (T, 3, 3) and f.min() >= 1 and f[..., 0].max() <= V and f[..., 1].max() <= 3 * T and f[..., 2].max() <= V
  assert np.array_equal(f[..., 0] - 1, m['faces']) and np.array_equal(f[..., 2], f[..., 0])
  assert np.array_equal(f[..., 1].reshape(-1) - 1, np.arange(3 * T))
  assert 'map_Kd scene.png' in open(str(tmp_path / 'scene.mtl')).read().split('\n')
  assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'scene.png'))), tex['texture'])
