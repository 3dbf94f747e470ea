"""View-dependent texture without a GPU: ops.sh_basis against the closed forms, the NumPy restatement (tests/shtex_ref.py) on an
exactly degree-2 colour field and on its fallbacks, the two deviations the GPU test's analytic bound is built from, the PLY / OBJ
round trip with and without SH, and render_mesh's default eye."""

import os

import numpy as np
import pytest

from multinerf_amd import mesh, ops
from tests import raster_ref as R
from tests import shtex_ref as S

F = np.float32
DIRS = mesh.sh_directions(2)


def test_direction_sets():
  assert DIRS.shape == (42, 3) and DIRS.dtype == F and mesh.sh_directions(3).shape == (92, 3)
  assert np.abs(np.linalg.norm(DIRS.astype(np.float64), axis=1) - 1).max() < 1e-7
  mine = mesh.sh_directions(np.array([[0, 0, 3.], [1, 1, 0]]))
  assert np.array_equal(mine, np.array([[0, 0, 1], [np.sqrt(0.5), np.sqrt(0.5), 0]], F))
  for bad in (np.zeros((2, 3)), np.zeros((0, 3)), np.ones((3, 2)), [[np.nan, 0, 1]]):
    with pytest.raises(ValueError):
      mesh.sh_directions(bad)


def test_basis_against_the_closed_forms_and_orthonormality():
  rng = np.random.default_rng(0)
  d = rng.normal(size=(500, 3))
  d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
  for degree in (0, 1, 2):
    Y = ops.sh_basis(d, degree)
    assert Y.dtype == np.float64 and Y.shape == (500, (degree + 1) ** 2)
    assert np.array_equal(Y, S.basis64(d, degree))
    dn = d.astype(np.float64)
    dn /= np.linalg.norm(dn, axis=1, keepdims=True)         # the closed forms take polar angles: of the exactly normalised direction
    assert np.abs(S._basis(dn, degree, np.float64) - S.closed_form(dn, degree)).max() < 1e-14
    assert np.abs(Y - S.closed_form(dn, degree)).max() < 1e-6          # float32 directions are unit to 6e-8
    assert np.abs(S.basis32(d, degree) - Y).max() < 5e-7
  # orthonormal under a quadrature that is exact for the products (degree 4): Gauss-Legendre in z, equal steps in the azimuth
  z, wz = np.polynomial.legendre.leggauss(8)
  ph = 2 * np.pi * (np.arange(16) + 0.5) / 16
  s = np.sqrt(1 - z * z)
  q = np.stack([s[:, None] * np.cos(ph), s[:, None] * np.sin(ph), z[:, None] * np.ones_like(ph)], -1).reshape(-1, 3)
  wq = np.repeat(wz, 16) * 2 * np.pi / 16
  Yq = S._basis(q, 2, np.float64)
  assert np.abs((Yq * wq[:, None]).T @ Yq - np.eye(9)).max() < 1e-14
  for bad in (3, -1, 1.5, True):
    with pytest.raises(ValueError):
      ops.sh_basis(d, bad)
  with pytest.raises(ValueError):
    ops.sh_basis(np.zeros((4, 2)), 1)


def _field_case(n=2000, seed=1):
  rng = np.random.default_rng(seed)
  p = rng.uniform(-1, 1, (n, 3))
  nrm = rng.normal(size=(n, 3))
  nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
  nrm[:6] = np.concatenate([np.eye(3), -np.eye(3)]).astype(F)        # orthogonal to some of the 42 directions exactly
  rgb = S.field_colour(np.repeat(p, len(DIRS), 0), np.tile(DIRS.astype(np.float64), (n, 1))).reshape(n, len(DIRS), 3).astype(F)
  return p, nrm, rgb


def test_the_restatement_recovers_a_degree_2_field_and_records_its_deviation():
  p, nrm, rgb = _field_case()
  assert rgb.min() > 0.05 and rgb.max() < 0.95 and (rgb.max(1) - rgb.min(1)).max() > 0.3    # nothing clips; the amplitude
  coef, status = S.fit(DIRS, nrm, rgb, 2, 0., return_status=True)
  assert (status == S.SOLVED).all()
  dev = float(np.abs(coef - S.field_coefficients(p)).max())
  print(f'largest coefficient deviation at lam = 0 on 42 directions: {dev:.3e}')
  assert S.FIT_DEVIATION / 4 <= dev <= S.FIT_DEVIATION, dev     # the recorded value holds, and is not a loose one
  # the ridge biases the coefficients, far above the deviation, but as the minimiser of sum_k w_k r_k^2 + mu |c_1..|^2 it cannot do
  # worse than the field's own coefficients, whose residual is 0: the objective at the fit is at most mu |c_1..|^2 of the field
  true = S.field_coefficients(p)
  ridge = S.fit(DIRS, nrm, rgb, 2, 1e-3).astype(np.float64)
  assert np.abs(ridge - true).max() > 10 * S.FIT_DEVIATION
  Y, w = S.basis64(DIRS, 2), S.weights(DIRS, nrm).astype(np.float64)
  mu = 1e-3 * (w[:, :, None] * Y[None] ** 2).sum((1, 2)) / 9
  r = np.einsum('dk,nkc->ndc', Y, ridge) - rgb
  objective = (w[:, :, None] * r * r).sum(1) + mu[:, None] * (ridge[:, 1:] ** 2).sum(1)
  assert (objective <= mu[:, None] * (true[:, 1:] ** 2).sum(1) * (1 + 1e-6) + 1e-12).all()
  # degrees 0 and 1 of their own fields
  for degree in (0, 1):
    rgb_d = S.field_colour(np.repeat(p, 42, 0), np.tile(DIRS.astype(np.float64), (len(p), 1)), degree).reshape(len(p), 42, 3).astype(F)
    assert np.abs(S.fit(DIRS, nrm, rgb_d, degree, 0.) - S.field_coefficients(p, degree)).max() <= S.FIT_DEVIATION


def test_the_float32_shading_error_of_the_restatement():
  """The float32 shading pass against the same formulas in float64 on the same float32 inputs (face, bary, uv, sh): the second term
  of the GPU test's bound."""
  m = S.icosphere_mesh(1)
  sh, uv, _ = S.bake(m, 5, DIRS, 2, 0., S.field_colour)
  worst = 0.
  for eye, focal in (((2.0, 1.2, 0.8), 40.), ((-0.3, 2.2, -1.0), 40.), ((0.1, -0.05, 0.15), 12.)):
    P = mesh.world_to_pixel(R.pixtocam(focal, 48, 40), R.look_at(eye, (0.02, -0.03, 0.01)))
    out = R.render(m, P, 40, 48, 1e-3)
    assert (out['face'] >= 0).sum() > 300
    a = S.shade(m['vertices'], m['faces'], out['face'], out['bary'], uv, sh, eye, out['rgb'])
    b = S.shade(m['vertices'], m['faces'], out['face'], out['bary'], uv, sh, np.asarray(eye, F), out['rgb'], F=np.float64)
    worst = max(worst, float(np.abs(a - b)[out['face'] >= 0].max()))
  print(f'largest float32 shading error: {worst:.3e}')
  assert S.SHADE_F32_ERROR / 4 <= worst <= S.SHADE_F32_ERROR, worst


def test_the_lookup_is_the_rasterisers():
  """tests/shtex_ref.py repeats the bilinear lookup of tests/raster_ref.py's `shade` (there it is no function of its own).  At degree 0
  with coefficients colour / C0 both must show the same image: a random texture (neighbouring texels differ by tenths) and UVs beyond
  [0, 1] (the clamps), to 8 float32 roundings of values up to 1 (the division, the product with C0, three lerps on either side)."""
  m = S.icosphere_mesh(1)
  rng = np.random.default_rng(12)
  tex = rng.uniform(0, 1, (13, 17, 3)).astype(F)
  uv = rng.uniform(-0.1, 1.1, (80, 3, 2)).astype(F)
  sh = (tex / F(S.C0))[:, :, None, :]
  for eye, focal in (((2.0, 1.2, 0.8), 40.), ((0.1, -0.05, 0.15), 12.)):
    P = mesh.world_to_pixel(R.pixtocam(focal, 48, 40), R.look_at(eye, (0.02, -0.03, 0.01)))
    out = R.render(m, P, 40, 48, 1e-3, texture=tex, uv=uv)
    got = S.shade(m['vertices'], m['faces'], out['face'], out['bary'], uv, sh, eye, np.ones((40, 48, 3), F))
    assert (out['face'] >= 0).sum() > 300 and np.abs(got - out['rgb']).max() <= 8 * 2. ** -24


def test_fallbacks():
  rng = np.random.default_rng(2)
  up = np.array([[0, 0, 1]], F)
  rgb = rng.uniform(0.1, 0.9, (1, 42, 3)).astype(F)
  seen = S.weights(DIRS, up)[0] > 0
  assert 0 < seen.sum() < 42 and S.weights(DIRS, up).max() <= 1
  # all directions skipped: a normal that is NaN or zero, or every visible colour not finite
  for nrm in (np.full((1, 3), np.nan, F), np.zeros((1, 3), F)):
    coef, status = S.fit(DIRS, nrm, rgb, 2, 1e-3, return_status=True)
    assert status[0] == S.EMPTY and not coef.any()
  bad = rgb.copy()
  bad[0, seen, 1] = np.inf
  coef, status = S.fit(DIRS, up, bad, 1, 0., return_status=True)
  assert status[0] == S.EMPTY and not coef.any()
  # what stands at a direction with weight 0 does not matter; a colour that is not finite is skipped, not propagated
  junk = rgb.copy()
  junk[0, ~seen] = np.nan
  assert np.array_equal(S.fit(DIRS, up, junk, 2, 1e-3), S.fit(DIRS, up, rgb, 2, 1e-3))
  one = rgb.copy()
  k = int(np.nonzero(seen)[0][3])
  one[0, k, 2] = np.nan
  coef, status = S.fit(DIRS, up, one, 2, 1e-3, return_status=True)
  assert status[0] == S.SOLVED and np.isfinite(coef).all()
  w = S.weights(DIRS, up).copy()
  less = np.delete(np.arange(42), k)
  assert np.array_equal(coef, S.fit(DIRS[less], up, rgb[:, less], 2, 1e-3))
  # D < K at lam = 0: one direction along -z, degree 1; the y and x columns of the table are exactly 0, so is the second pivot
  d1 = np.array([[0, 0, -1]], F)
  c1 = np.array([[[0.2, 0.4, 0.6]]], F)
  coef, status = S.fit(d1, up, c1, 1, 0., return_status=True)
  assert status[0] == S.MEAN and not coef[0, 1:].any()
  assert np.array_equal(coef[0, 0], ((c1[0, 0].astype(np.float64) / 1.) / S.C0).astype(F))
  assert np.abs(coef[0, 0] * S.C0 - c1[0, 0]).max() < 1e-7   # the constant alone reproduces the mean colour
  # with the ridge the same texel is solvable, and degree 0 always is
  assert S.fit(d1, up, c1, 1, 1e-3, return_status=True)[1][0] == S.SOLVED
  assert S.fit(d1, up, c1, 0, 0., return_status=True)[1][0] == S.SOLVED
  # a generic D < K: whatever the rounding makes of the singular matrix, the output is finite
  few = DIRS[seen][:5]
  coef = S.fit(few, up, rgb[:, :5], 2, 0.)
  assert np.isfinite(coef).all()
  # colours near the float32 maximum: the sums are float64, the mean that does not fit float32 becomes 0
  huge = np.full((1, 1, 3), 3e38, F)
  coef, status = S.fit(d1, up, huge, 1, 0., return_status=True)
  assert status[0] == S.MEAN and not coef.any()


def _tiny_mesh():
  v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
  n = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 1]], F)
  return dict(vertices=v, normals=n, faces=np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.int32))


def _tiny_texture(degree=None):
  rng = np.random.default_rng(4)
  lay = ops.atlas_layout(3, 3)
  t = dict(texture=rng.integers(0, 256, (lay['H'], lay['W'], 3)).astype(np.uint8), uv=rng.uniform(0, 1, (3, 3, 2)).astype(F))
  if degree is not None:
    t['sh'] = rng.normal(size=(lay['H'], lay['W'], (degree + 1) ** 2, 3)).astype(F)
    t['sh'][0, 0, 0, 0] = 1e6                                # beyond float16
  return t


def _files(d):
  return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize('sh_dtype', mesh.SH_DTYPES)
def test_file_round_trip(tmp_path, sh_dtype):
  m = _tiny_mesh()
  plain, with_sh = tmp_path / 'plain', tmp_path / 'sh'
  plain.mkdir(), with_sh.mkdir()
  mesh.write_ply(str(plain / 'a.ply'), m, texture=_tiny_texture())
  mesh.write_obj(str(plain / 'b.obj'), m, _tiny_texture())
  t = _tiny_texture(1)
  mesh.write_ply(str(with_sh / 'a.ply'), m, texture=t, sh_dtype=sh_dtype)
  mesh.write_obj(str(with_sh / 'b.obj'), m, t, sh_dtype=sh_dtype)
  a, b = _files(str(plain)), _files(str(with_sh))
  assert sorted(a) == ['a.ply', 'a.png', 'b.mtl', 'b.obj', 'b.png'] and sorted(set(b) - set(a)) == ['a_sh.npy', 'b_sh.npy']
  # without SH the files are the existing writer's; with SH everything but the PLY header's one line is
  for name in ('a.png', 'b.mtl', 'b.obj', 'b.png'):
    assert a[name] == b[name], name
  line = b'comment TextureSH a_sh.npy 1\n'
  assert line not in a['a.ply'] and b['a.ply'].count(line) == 1 and b['a.ply'].replace(line, b'') == a['a.ply']
  assert b['a.ply'].index(b'comment TextureFile a.png\n') < b['a.ply'].index(line) < b['a.ply'].index(b'element vertex')
  assert b['a_sh.npy'] == b['b_sh.npy']
  stored = np.load(str(with_sh / 'a_sh.npy'))
  assert stored.dtype == np.dtype(sh_dtype) and stored.shape == t['sh'].shape
  want = t['sh'] if sh_dtype == 'float32' else np.clip(t['sh'], -65504, 65504).astype(np.float16)
  assert np.array_equal(stored, want)
  back = mesh.read_ply(str(with_sh / 'a.ply'))
  assert back['texture_sh'].dtype == F and np.array_equal(back['texture_sh'], want.astype(F)) and back['texture_sh_file'] == 'a_sh.npy'
  assert back['texture_file'] == 'a.png' and np.array_equal(back['texcoord'], t['uv']) and np.array_equal(back['faces'], m['faces'])
  if sh_dtype == 'float16':
    small = np.abs(t['sh']) < 6e4
    assert (np.abs(back['texture_sh'] - t['sh'])[small] <= 2. ** -11 * np.abs(t['sh'])[small] + 2. ** -25).all()
  plain_back = mesh.read_ply(str(plain / 'a.ply'))
  assert 'texture_sh' not in plain_back and plain_back['texture_file'] == 'a.png'
  # the line without the file: the plain texture is what is left
  os.remove(str(with_sh / 'a_sh.npy'))
  assert 'texture_sh' not in mesh.read_ply(str(with_sh / 'a.ply'))
  with pytest.raises(ValueError):
    mesh.write_ply(str(with_sh / 'c.ply'), m, texture=t, sh_dtype='bfloat16')
  with pytest.raises(ValueError):
    mesh.write_ply(str(with_sh / 'c.ply'), m, texture=dict(t, sh=t['sh'][:, :, :3]))


def test_untextured_ply_is_unchanged(tmp_path):
  m = _tiny_mesh()
  mesh.write_ply(str(tmp_path / 'a.ply'), m)
  mesh.write_ply(str(tmp_path / 'b.ply'), m, sh_dtype='float32')
  assert open(str(tmp_path / 'a.ply'), 'rb').read() == open(str(tmp_path / 'b.ply'), 'rb').read()
  assert sorted(os.listdir(str(tmp_path))) == ['a.ply', 'b.ply']


def test_default_origin_of_a_projection():
  rng = np.random.default_rng(6)
  for eye in ((2.0, 1.2, 0.8), (0.1, -0.05, 0.15), (-30., 4., 11.)):
    c2w = R.look_at(eye, rng.uniform(-0.2, 0.2, 3))
    K = np.linalg.inv(R.pixtocam(37.5, 48, 40))
    w2c = np.concatenate([c2w[:, :3].T, -(c2w[:, :3].T @ c2w[:, 3])[:, None]], 1)
    P = K @ np.diag([1., -1., -1.]) @ w2c                    # world_to_pixel's matrix before its rounding to float32
    o = mesh.projection_origin(P)
    assert o.dtype == np.float64 and np.abs(o - c2w[:3, 3]).max() <= 1e-13 * np.abs(c2w[:3, 3]).max()
    assert np.abs(mesh.projection_origin(mesh.world_to_pixel(R.pixtocam(37.5, 48, 40), c2w)) - c2w[:3, 3]).max() < 1e-5 * np.abs(c2w[:3, 3]).max()
    assert np.array_equal(mesh.projection_origin(2.5 * P), mesh.projection_origin(2.5 * P)) and np.abs(mesh.projection_origin(2.5 * P) - o).max() < 1e-12
  for bad in (np.zeros((3, 4)), np.concatenate([np.ones((3, 3)), np.zeros((3, 1))], 1), np.full((3, 4), np.nan)):
    with pytest.raises(ValueError):
      mesh.projection_origin(bad)
