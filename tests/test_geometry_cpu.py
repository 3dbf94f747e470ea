"""The NumPy restatement of the mesh-geometry kernels (tests/geometry_ref.py) against known answers, without a GPU: the float64 form
against dense barycentric sampling and against plain point and segment distances on degenerate faces, the float32 form against the
float64 form on exactly the inputs of tests/test_gpu_geometry.py (the deviation is what that file's float64 tolerance is four times
of; profiles/mesh_geometry.md records it), the integer mix, and mesh.read_ply_geometry on files written here."""

import numpy as np
import pytest

from tests import geometry_ref as G

F32, F64 = np.float32, np.float64


def test_float64_form_against_dense_sampling():
  rng = np.random.default_rng(1)
  steps = 200
  for _ in range(4):
    a, b, c = rng.uniform(-0.6, 0.6, (3, 3))
    p = rng.uniform(-1., 1., (300, 3))
    d = np.sqrt(G.face_d2(p, a, b, c))
    sampled = G.sampled_triangle(p, a, b, c, steps)
    step = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)) / steps
    assert (d <= sampled + 1e-12).all() and (sampled - d <= step).all()      # a lower bound of the sampled distance, within the step


def test_degenerate_faces_are_points_and_segments():
  rng = np.random.default_rng(2)
  p = rng.uniform(-1., 1., (500, 3))
  a, b = rng.uniform(-0.6, 0.6, (2, 3))
  point = np.linalg.norm(p - a, axis=-1)
  assert np.allclose(np.sqrt(G.face_d2(p, a, a, a)), point, rtol=0, atol=1e-14)
  seg = G.point_segment(p, a, b)
  far = a + 3. * (b - a)
  for tri, want in (((a, a, b), seg), ((a, b, b), seg), ((b, a, b), seg), ((a, b, a + 0.25 * (b - a)), seg), ((a, b, far), G.point_segment(p, a, far))):
    got = np.sqrt(G.face_d2(p, *tri))
    assert np.isfinite(got).all() and np.abs(got - want).max() < 1e-9
  # float32, the collinear face of the soup and its equal-corner faces: finite, and the segment / point distance to rounding
  verts, faces = G.soup()
  q = rng.uniform(-1., 1., (500, 3)).astype(F32)
  A, B, C = (verts[faces[62, k]] for k in range(3))
  assert np.abs(np.sqrt(G.face_d2(q, A, B, C).astype(F64)) - G.point_segment(q, A, C)).max() < 1e-6
  A = verts[faces[60, 0]]
  assert (verts[faces[60]] == A).all()
  assert np.abs(np.sqrt(G.face_d2(q, A, A, A).astype(F64)) - np.linalg.norm(q.astype(F64) - A.astype(F64), axis=-1)).max() < 1e-6
  A, B, C = (verts[faces[61, k]] for k in range(3))
  assert np.abs(np.sqrt(G.face_d2(q, A, B, C).astype(F64)) - G.point_segment(q, A, C)).max() < 1e-6


@pytest.mark.parametrize('flat', [False, True], ids=['soup', 'flat'])
def test_float32_form_against_float64_on_the_gpu_tests_inputs(flat):
  verts, faces = G.soup(flat=flat)
  lo, hi = G.soup_box(verts, faces)
  q = G.queries(verts, faces, float(F32((hi - lo).max() / 20)))
  assert q.shape == (1500, 3) and q.dtype == F32 and len(faces) == 300 and G.valid_faces(verts, faces).sum() == 296
  d32, f32 = G.point_mesh_distance(q, verts, faces)
  d64, f64 = G.point_mesh_distance(q, verts, faces, dtype=F64)
  assert d32.dtype == F32 and d64.dtype == F64
  live = np.isfinite(q).all(1)
  assert (f32[~live] == -1).all() and np.isinf(d32[~live]).all() and (f32[live] >= 0).all()
  diff = np.zeros(len(q))
  diff[live] = np.abs(np.sqrt(d32[live].astype(F64)) - np.sqrt(d64[live]))
  dev = diff[live]
  sliver = np.isin(f64, np.arange(70, 120)) | np.isin(f32, np.arange(70, 120))
  print(f'float32 against float64, distance: {dev.max():.3e} over all queries, {dev[~sliver[live]].max():.3e} where no sliver is nearest; '
        f'relative to the distance {np.max(dev / np.maximum(np.sqrt(d64[live]), 1e-3)):.3e}')
  # float32 has 24 bits: a distance of the size of the box (queries at 50 apart) carries 50 * 2^-24 * a few operations
  near = live & (np.sqrt(d64) < 2.)
  assert diff[near].max() < 1e-4
  assert (diff[live] <= 1e-4 + 64 * 2. ** -24 * np.sqrt(d64[live])).all()
  # ties and max_dist follow the stated rules
  assert not np.isin(f32, np.arange(50, 60)).any()
  cut32 = G.point_mesh_distance(q, verts, faces, max_dist=0.05)
  inside = d32 <= F32(0.05) * F32(0.05)
  assert np.array_equal(cut32[1] >= 0, inside) and np.array_equal(cut32[0][inside], d32[inside]) and np.array_equal(cut32[1][inside], f32[inside])


def test_integer_mix_known_answers():
  # x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, by hand (Python integers, masked to 32 bits)
  def by_hand(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x
  known = {0: 0x0, 1: 0x688990c0, 2: 0xd1132181, 0xffffffff: 0x6768824a, 0x9e3779b9: 0x1fce552, 123456789: 0xa8f1db88}
  for x, want in known.items():
    assert by_hand(x) == want and int(G.mix(np.uint32(x))) == want
  assert np.array_equal(G.mix(np.array(list(known), dtype=np.uint32)), np.array(list(known.values()), dtype=np.uint32))
  assert int(G.mix(np.uint32(0))) == 0                                       # the mix fixes 0: the seed is mixed first, then added to
  got = G.mix(np.arange(1 << 16, dtype=np.uint32))
  assert len(np.unique(got)) == 1 << 16                                       # a bijection on what we can enumerate
  b = G.barycentrics(5000, 0)
  assert b.dtype == F32 and (b >= 0).all() and (b <= 1).all() and (b.sum(1) == 1).all()
  assert not np.array_equal(b, G.barycentrics(5000, 1))
  assert np.abs(b.mean(0) - 1 / 3).max() <= 6 * np.sqrt(1 / (18 * 5000))


def test_restated_sampler_is_stratified():
  verts = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1], [1, 1, 1], [2, 2, 2], [3, 3, 3]], F32)
  faces = np.array([[0, 1, 2], [6, 7, 8], [3, 4, 5], [0, 1, 9]], np.int32)
  area = G.face_areas(verts, faces)
  assert area.tolist() == [1., 0., 3., 0.]
  pts, face, b = G.sample(verts, faces, np.cumsum(area), 1001, 5)
  count = np.bincount(face, minlength=4)
  assert count[1] == count[3] == 0 and abs(count[0] - 1001 / 4) <= 2 and abs(count[2] - 3 * 1001 / 4) <= 2
  assert ((pts[:, 2] == 0) == (face == 0)).all()


# ---- read_ply_geometry

def ply(tmp_path, name, header, body, binary):
  path = str(tmp_path / name)
  with open(path, 'wb') as f:
    f.write(('ply\nformat ' + ('binary_little_endian' if binary else 'ascii') + ' 1.0\ncomment made by a test\n' + header + 'end_header\n').encode())
    f.write(body if binary else body.encode())
  return path


def test_read_ply_geometry(tmp_path):
  from multinerf_amd import mesh
  v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.25, 1.5]], F64)
  tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
  # ascii, floats, with faces (vertex_index) and an extra face scalar
  rows = ''.join(f'{x} {y} {z}\n' for x, y, z in v) + ''.join(f'3 {a} {b} {c} 7\n' for a, b, c in tri)
  m = mesh.read_ply_geometry(ply(tmp_path, 'a.ply', 'element vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
                                 'element face 2\nproperty list uchar int vertex_index\nproperty uchar flags\n', rows, False))
  assert np.array_equal(m['vertices'], v.astype(F32)) and np.array_equal(m['faces'], tri) and m['normals'] is None and m['colors'] is None
  assert m['vertices'].dtype == F32 and m['faces'].dtype == np.int32
  # binary, doubles, normals, colours, extra scalars before and after, uint indices, an element that follows
  vt = np.dtype([('q', '<f4'), ('x', '<f8'), ('y', '<f8'), ('z', '<f8'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'), ('red', 'u1'),
                 ('green', 'u1'), ('blue', 'u1'), ('alpha', 'u1'), ('label', '<i2')])
  rec = np.zeros((4,), vt)
  rec['x'], rec['y'], rec['z'] = v.T
  rec['nz'], rec['red'], rec['blue'], rec['q'], rec['label'] = 1, 200, 17, 3.5, -2
  ft = np.dtype([('n', 'u1'), ('v', '<u4', (3,))])
  frec = np.zeros((2,), ft)
  frec['n'], frec['v'] = 3, tri
  header = ('element vertex 4\nproperty float q\nproperty double x\nproperty double y\nproperty double z\nproperty float nx\nproperty float ny\n'
            'property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nproperty short label\n'
            'element face 2\nproperty list uchar uint vertex_indices\nelement edge 1\nproperty int a\nproperty int b\n')
  m = mesh.read_ply_geometry(ply(tmp_path, 'b.ply', header, rec.tobytes() + frec.tobytes() + np.zeros(2, '<i4').tobytes(), True))
  assert np.array_equal(m['vertices'], v.astype(F32)) and np.array_equal(m['faces'], tri)
  assert np.array_equal(m['normals'], np.tile(F32([0, 0, 1]), (4, 1))) and np.array_equal(m['colors'], np.tile(np.uint8([200, 0, 17]), (4, 1)))
  # no faces: a point cloud, ascii doubles and binary floats
  m = mesh.read_ply_geometry(ply(tmp_path, 'c.ply', 'element vertex 4\nproperty double x\nproperty double y\nproperty double z\n',
                                 ''.join(f'{float(x)!r} {float(y)!r} {float(z)!r}\n' for x, y, z in v), False))
  assert np.array_equal(m['vertices'], v.astype(F32)) and m['faces'].shape == (0, 3) and m['faces'].dtype == np.int32
  m = mesh.read_ply_geometry(ply(tmp_path, 'd.ply', 'element vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 0\n'
                                 'property list uchar int vertex_indices\n', v.astype('<f4').tobytes(), True))
  assert np.array_equal(m['vertices'], v.astype(F32)) and m['faces'].shape == (0, 3)
  # what mesh.write_ply writes, textured or not, reads back
  path = str(tmp_path / 'e.ply')
  mesh.write_ply(path, dict(vertices=v.astype(F32), normals=np.tile(F32([0, 0, 1]), (4, 1)), faces=tri, colors=np.full((4, 3), 9, np.uint8)))
  m = mesh.read_ply_geometry(path)
  assert np.array_equal(m['vertices'], v.astype(F32)) and np.array_equal(m['faces'], tri) and (m['colors'] == 9).all()
  # refused, naming what was met
  xyz = 'element vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
  quad = np.zeros((1,), np.dtype([('n', 'u1'), ('v', '<i4', (4,))]))
  quad['n'], quad['v'] = 4, [0, 1, 3, 2]
  with pytest.raises(ValueError, match='4 vertices'):
    mesh.read_ply_geometry(ply(tmp_path, 'f.ply', xyz + 'element face 1\nproperty list uchar int vertex_indices\n', v.astype('<f4').tobytes() + quad.tobytes(), True))
  with pytest.raises(ValueError, match='4 vertices|triangles'):
    mesh.read_ply_geometry(ply(tmp_path, 'g.ply', xyz + 'element face 1\nproperty list uchar int vertex_indices\n',
                               ''.join(f'{x} {y} {z}\n' for x, y, z in v) + '4 0 1 3 2\n', False))
  with pytest.raises(ValueError, match='big_endian'):
    path = ply(tmp_path, 'h.ply', xyz, '', False)
    text = open(path, 'rb').read().replace(b'ascii', b'binary_big_endian')
    open(path, 'wb').write(text)
    mesh.read_ply_geometry(path)
  with pytest.raises(ValueError, match='x y z'):
    mesh.read_ply_geometry(ply(tmp_path, 'i.ply', 'element vertex 1\nproperty float x\nproperty float y\n', '0 0\n', False))
  with pytest.raises(ValueError, match='x y z'):
    mesh.read_ply_geometry(ply(tmp_path, 'j.ply', 'element vertex 1\nproperty int x\nproperty int y\nproperty int z\n', '0 0 0\n', False))
  with pytest.raises(ValueError, match='outside'):
    mesh.read_ply_geometry(ply(tmp_path, 'k.ply', xyz + 'element face 1\nproperty list uchar int vertex_indices\n',
                               ''.join(f'{x} {y} {z}\n' for x, y, z in v) + '3 0 1 4\n', False))
  with pytest.raises(ValueError, match='list property'):
    mesh.read_ply_geometry(ply(tmp_path, 'l.ply', 'element vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty list uchar int n\n',
                               '0 0 0 0\n', False))
  with pytest.raises(ValueError, match='not a PLY'):
    open(str(tmp_path / 'm.ply'), 'wb').write(b'solid\n')
    mesh.read_ply_geometry(str(tmp_path / 'm.ply'))
