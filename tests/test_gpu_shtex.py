"""View-dependent texture on the GPU (-m gpu): the kernels of csrc/shtex.hip through ops.shtex_weights / shtex_fit / shtex_shade,
mesh.bake_texture(sh_degree=) and mesh.render_mesh against the NumPy restatement (tests/shtex_ref.py) bit for bit, an exactly
degree-2 colour field end to end against its own values (bound from tests/test_shtex_cpu.py's two recorded deviations), the
invariances, a small Ref-NeRF model, and the two scripts.  Measured figures are in profiles/texture_sh.md."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import atlas_ref as A
from tests import raster_ref as R
from tests import shtex_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DIRS = {12: mesh.sh_directions(1), 42: mesh.sh_directions(2)}
SIZES = ((40, 48), (5, 7))         # H, W: 1920 pixels are 7.5 workgroups, 35 less than one
# eye, target, focal of a 48-wide image; the last eye is inside the sphere of radius 0.8
VIEWS = (((2.0, 1.2, 0.8), (0.02, -0.03, 0.01), 40.), ((-0.3, 2.2, -1.0), (0.02, -0.03, 0.01), 40.), ((0.1, -0.05, 0.15), (1., 0.3, 0.2), 12.))
# The analytic bound (tests/shtex_ref.py records both terms, tests/test_shtex_cpu.py asserts them): the coefficients' deviation
# through the basis, plus the float32 shading error, times 4 for the rounding of the bilinear weights and of the interpolated
# position, which the two terms were not measured with.  (5.0e-7 x 4.564 + 2.5e-7) x 4 = 1.01e-5.
BOUND = 4 * (S.FIT_DEVIATION * S.SUM_MAX_BASIS + S.SHADE_F32_ERROR)


def bits(a):
  a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
  return a.view(np.uint32) if a.dtype == np.float32 else a


def to_device(m):
  return {k: torch.from_numpy(np.array(m[k])).cuda() for k in ('vertices', 'normals', 'faces')}


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def soup():
  """31 random triangles (an odd count: the last cell has a spare half) that intersect each other; vertex 4 is NaN, face 7 is a
  sliver (its third corner 1e-7 off the line through the other two), face 9 has zero vertex normals."""
  rng = np.random.default_rng(8)
  T = 31
  v = rng.uniform(-0.6, 0.6, (3 * T, 3)).astype(F)
  n = rng.normal(size=(3 * T, 3)).astype(F)
  v[4] = np.nan
  v[23] = v[21] + F(0.37) * (v[22] - v[21]) + F(1e-7)
  n[27:30] = 0
  return dict(vertices=v, normals=n, faces=np.arange(3 * T, dtype=np.int32).reshape(T, 3))


@functools.lru_cache(maxsize=None)
def source(name):
  m = soup() if name == 'soup' else S.icosphere_mesh(dict(ico80=1, ico320=2)[name])
  for a in m.values():
    a.setflags(write=False)
  return m


def projection(view, H, W):
  eye, target, focal = VIEWS[view]
  return mesh.world_to_pixel(R.pixtocam(focal * W / 48., W, H), R.look_at(eye, target)), np.asarray(eye, np.float64)


def normals_case(n, seed=0):
  rng = np.random.default_rng(seed)
  nrm = rng.normal(size=(n, 3))
  nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
  special = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [np.nan, 0, 0], [0, 0, 0], [3, 0, 0]], F)   # axes: orthogonal to some
  k = min(n, len(special))                                                                                      # directions exactly
  nrm[:k] = special[:k] if n > 1 else special[2:3]
  return nrm


# ---- the three kernels against the restatement, bit for bit

@pytest.mark.parametrize('D', (12, 42))
@pytest.mark.parametrize('n', (1, 301))
def test_weights_against_the_restatement(D, n):
  nrm = normals_case(n)
  w = ops.shtex_weights(dev(DIRS[D]), dev(nrm))
  want = S.weights(DIRS[D], nrm)
  assert tuple(w.shape) == (n, D) and np.array_equal(bits(w), bits(want))
  if n > 1:
    assert (want[:4] == 0).sum() > (4 * D) // 2 and (want[4:6] == 0).all() and want.max() == 1        # exact zeros beyond the back half


def fit_case(D, n, seed=1):
  """Random colours with every fallback in it (n >= 12): texel 4 and 5 see nothing (NaN and zero normal), 7 has no finite visible
  colour, 8 one NaN channel, 9 infinities at directions it does not see, 10 colours near the float32 maximum, 11 a single finite
  visible colour."""
  rng = np.random.default_rng(seed)
  nrm = normals_case(n)
  rgb = rng.uniform(0, 1, (n, D, 3)).astype(F)
  if n >= 12:
    w = S.weights(DIRS[D], nrm)
    rgb[7][w[7] > 0] = np.nan
    rgb[8, int(np.nonzero(w[8] > 0)[0][0]), 1] = np.nan
    rgb[9][w[9] == 0] = np.inf
    rgb[10] = F(3e38)
    rgb[11][np.nonzero(w[11] > 0)[0][1:]] = -np.inf
  return nrm, rgb


@pytest.mark.parametrize('lam', (0., 1e-3))
@pytest.mark.parametrize('degree', (0, 1, 2))
@pytest.mark.parametrize('D', (12, 42))
def test_fit_against_the_restatement(D, degree, lam):
  for n in (1, 301):                                        # one lane of one workgroup; 2 workgroups and 45 lanes of a third
    nrm, rgb = fit_case(D, n)
    coef = ops.shtex_fit(dev(DIRS[D]), dev(nrm), dev(rgb), degree, lam)
    want, status = S.fit(DIRS[D], nrm, rgb, degree, lam, return_status=True)
    assert tuple(coef.shape) == (n, (degree + 1) ** 2, 3) and bool(torch.isfinite(coef).all())
    same = np.array_equal(bits(coef), bits(want))
    assert same, (np.abs(coef.cpu().numpy() - want).max(), np.nonzero((bits(coef) != bits(want)).any((1, 2)))[0][:10], status[:12])
    if n > 1:
      assert (status[[4, 5, 7]] == S.EMPTY).all() and (status[[8, 9, 10, 11]] != S.EMPTY).all()
      if degree == 2 and lam == 0 and D == 12:             # at most 6 of the 12 directions are seen, fewer than K = 9: every system
        assert (S.weights(DIRS[D], nrm) > 0).sum(1).max() < 9                        # is singular, what the rounding makes of it is finite
      else:
        assert status[8] == S.SOLVED and status[9] == S.SOLVED and (status == S.SOLVED).sum() > n - 12
  again = ops.shtex_fit(dev(DIRS[D]), dev(nrm), dev(rgb), degree, lam)
  assert torch.equal(again.view(torch.int32), coef.view(torch.int32))


def test_fit_falls_back_to_the_mean_colour():
  """One direction along -z for the normal +z at degree 1 and lam = 0: the second pivot is exactly 0."""
  d1, up, c1 = np.array([[0, 0, -1]], F), np.array([[0, 0, 1]], F), np.array([[[0.2, 0.4, 0.6]]], F)
  coef = ops.shtex_fit(dev(d1), dev(up), dev(c1), 1, 0.)
  want, status = S.fit(d1, up, c1, 1, 0., return_status=True)
  assert status[0] == S.MEAN and np.array_equal(bits(coef), bits(want)) and not want[0, 1:].any() and np.abs(want[0, 0] * S.C0 - c1[0, 0]).max() < 1e-7


def test_argument_checks():
  d, nrm, rgb = dev(DIRS[12]), dev(normals_case(5)), torch.zeros((5, 12, 3)).cuda()
  for bad in (lambda: ops.shtex_fit(d, nrm, rgb, 3), lambda: ops.shtex_fit(d, nrm, rgb, -1), lambda: ops.shtex_fit(d, nrm, rgb, 1, lam=-1e-3),
              lambda: ops.shtex_fit(d, nrm, rgb, 1, lam=float('nan')), lambda: ops.shtex_fit(d, nrm, rgb, 1, lam=float('inf')),
              lambda: ops.shtex_fit(d, nrm, rgb[:, :11].contiguous(), 1), lambda: ops.shtex_fit(d[:0], nrm, rgb[:, :0].contiguous(), 1),
              lambda: ops.shtex_fit(d, nrm, rgb.double(), 1), lambda: ops.shtex_fit(d, nrm, rgb, 1, basis=torch.zeros((12, 9), dtype=torch.float64).cuda()),
              lambda: ops.shtex_weights(d[:0], nrm), lambda: ops.shtex_weights(d, nrm[:, :2].contiguous()), lambda: ops.shtex_weights(d.double(), nrm),
              lambda: ops.shtex_weights(torch.zeros((513, 3)).cuda(), nrm)):
    with pytest.raises(ValueError):
      bad()
  assert tuple(ops.shtex_fit(d, nrm[:0], rgb[:0], 2).shape) == (0, 9, 3) and tuple(ops.shtex_weights(d, nrm[:0]).shape) == (0, 12)
  m = to_device(source('ico80'))
  face, bary = torch.zeros((5, 7), dtype=torch.int32).cuda(), torch.zeros((5, 7, 3)).cuda()
  uv, sh, out = torch.zeros((80, 3, 2)).cuda(), torch.zeros((4, 4, 4, 3)).cuda(), torch.zeros((5, 7, 3)).cuda()
  for bad in (lambda: ops.shtex_shade(m, face, bary, uv, sh[:, :, :3].contiguous(), (0, 0, 3), out), lambda: ops.shtex_shade(m, face, bary, uv[:79], sh, (0, 0, 3), out),
              lambda: ops.shtex_shade(m, face, bary, uv, sh, (0, float('nan'), 3), out), lambda: ops.shtex_shade(m, face, bary, uv, sh, (0, 0, 3), out[:4]),
              lambda: ops.shtex_shade(m, face.long(), bary, uv, sh, (0, 0, 3), out), lambda: ops.shtex_shade(m, face, bary, uv, sh.half(), (0, 0, 3), out)):
    with pytest.raises(ValueError):
      bad()
  with pytest.raises(ValueError):
    mesh.bake_texture(m, color_fn=lambda *a: None, cell=3, sh_degree=3)
  with pytest.raises(ValueError):
    mesh.bake_texture(m, color_fn=lambda *a: None, cell=3, sh_degree=1, sh_lambda=-1.)
  with pytest.raises(ValueError):
    mesh.render_mesh(m, None, None, 5, 7, texture=dict(texture=torch.zeros((4, 4, 3)).cuda(), uv=uv, sh=sh), proj=np.zeros((3, 4), F))


@pytest.mark.parametrize('degree', (0, 1, 2))
@pytest.mark.parametrize('name,cell', [('ico80', 5), ('ico320', 3), ('soup', 3)])
def test_shade_against_the_restatement(name, cell, degree):
  """Random coefficients (a NaN, an infinity and values far outside [0, 1] among them: the clamps) on the atlas's own UVs, for the soup
  UVs beyond [0, 1]; face and bary are the rasteriser's."""
  m = source(name)
  dm = to_device(m)
  T = len(m['faces'])
  lay = A.layout(T, cell)
  rng = np.random.default_rng(T + degree)
  sh = rng.normal(0, 0.6, (lay['H'], lay['W'], (degree + 1) ** 2, 3)).astype(F)
  sh[1, 2, 0, 0], sh[2, 1, 0, 1], sh[0, 0] = np.nan, np.inf, 50.
  uv = rng.uniform(-0.1, 1.1, (T, 3, 2)).astype(F) if name == 'soup' else A.uvs(T, lay)
  shaded = 0
  for H, W in SIZES:
    for view in range(len(VIEWS)):
      P, eye = projection(view, H, W)
      vis = ops.raster_visibility(dm, P, H, W, 1e-3)
      out = ops.raster_shade(dm, P, vis, 1e-3, bg=(0.25, 0.5, 0.75))
      face, bary, before = out['face'].cpu().numpy(), out['bary'].cpu().numpy(), out['rgb'].cpu().numpy()
      got = ops.shtex_shade(dm, out['face'], out['bary'], dev(uv), dev(sh), eye, out['rgb'])
      assert got is out['rgb']
      want = S.shade(m['vertices'], m['faces'], face, bary, uv, sh, eye, before)
      assert np.array_equal(bits(got), bits(want)), (name, H, W, view, np.nanmax(np.abs(got.cpu().numpy() - want)))
      assert np.array_equal(bits(got.cpu().numpy()[face < 0]), bits(before[face < 0])) and np.isfinite(want).all()
      assert want.min() >= 0 and want.max() <= 1
      shaded += int((face >= 0).sum())
  assert shaded > 1500
  # a face id beyond the mesh, and an eye on the surface point itself, leave the pixel alone resp. look along (0, 0, 1)
  face = torch.full((1, 2), T, dtype=torch.int32).cuda()
  face[0, 1] = 0
  bary = torch.tensor([[[0.2, 0.3, 0.5], [1., 0., 0.]]]).cuda()
  rgb = torch.full((1, 2, 3), 0.125).cuda()
  eye = m['vertices'][m['faces'][0, 0]]
  ops.shtex_shade(dm, face, bary, dev(uv), dev(sh), eye, rgb)
  want = S.shade(m['vertices'], m['faces'], face.cpu().numpy(), bary.cpu().numpy(), uv, sh, eye, np.full((1, 2, 3), 0.125, F))
  assert np.array_equal(bits(rgb), bits(want)) and (want[0, 0] == 0.125).all()


# ---- an exactly degree-2 colour field, end to end

def field_color_fn(degree=2, seed=3):
  def color_fn(means, covs, normals, viewdirs):
    rgb = S.field_colour(means.cpu().numpy(), viewdirs.cpu().numpy(), degree, seed)
    return torch.from_numpy(rgb.astype(F)).to(means.device)
  return color_fn


@functools.lru_cache(maxsize=None)
def field_bake(name, cell, D):
  return mesh.bake_texture(to_device(source(name)), color_fn=field_color_fn(), cell=cell, filter=0., sh_degree=2, sh_dirs=DIRS[D], sh_lambda=0.,
                           return_float=True)


@pytest.mark.parametrize('name,cell', [('ico80', 5), ('ico320', 3)])
def test_analytic_field_end_to_end(name, cell):
  """The bake at lam = 0 recovers the field, and a render shows, at every pixel, the field at that pixel's own surface point and view
  direction to BOUND; the head-on texture misses it by far more.  This fails without the feature."""
  m = source(name)
  dm = to_device(m)
  baked = field_bake(name, cell, 42)
  assert baked['sh_degree'] == 2 and tuple(baked['sh_dirs'].shape) == (42, 3) and 0 < baked['sh_queries'] <= 21 * int((baked['mask'] == 255).sum())
  want_sh, want_uv, _ = S.bake(m, cell, DIRS[42], 2, 0., S.field_colour)
  assert np.array_equal(bits(baked['sh']), bits(want_sh)) and np.array_equal(bits(baked['uv']), bits(want_uv))
  worst = worst_plain = 0.
  for view in range(len(VIEWS)):
    H, W = SIZES[0]
    P, eye = projection(view, H, W)
    r = mesh.render_mesh(dm, None, None, H, W, texture=baked, proj=P, near=1e-3)
    plain = mesh.render_mesh(dm, None, None, H, W, texture=baked, proj=P, near=1e-3, view_dependent=False)
    face, bary = r['face'].cpu().numpy(), r['bary'].cpu().numpy()
    origin = mesh.projection_origin(P)
    assert np.abs(origin - eye).max() < 1e-5
    # the pixel's own X and d, in float64 from the rasteriser's barycentrics
    _, (ys, xs, X, d) = S.shade(m['vertices'], m['faces'], face, bary, want_uv, want_sh, origin.astype(F), np.zeros((H, W, 3)), F=np.float64,
                                return_points=True)
    assert len(ys) > 300
    truth = S.field_colour(X, d)
    assert truth.min() > 0.02 and truth.max() < 0.98         # nothing clips
    err = np.abs(r['rgb'].cpu().numpy()[ys, xs] - truth)
    err_plain = plain['rgb'].cpu().numpy()[ys, xs] - truth
    rms_plain = float(np.sqrt((err_plain ** 2).mean()))
    print(f'{name} cell {cell} view {view}: {len(ys)} pixels, sh max error {err.max():.3e} (bound {BOUND:.3e}), head-on rms error {rms_plain:.3e}')
    assert err.max() <= BOUND
    assert rms_plain > err.max() and rms_plain > 100 * BOUND
    worst, worst_plain = max(worst, float(err.max())), max(worst_plain, rms_plain)


def test_direction_independent_colour():
  """A colour that ignores the view direction: the coefficients beyond the constant are rounding (0 to 1e-9; the bits are the
  restatement's), and the render is the plain float texture's to BOUND."""
  m = source('ico80')
  dm = to_device(m)
  flat = lambda p, d: 0.5 + 0.3 * np.asarray(p, np.float64) @ np.array([[0.9, 0.1, -0.3], [0.2, -0.8, 0.4], [-0.5, 0.3, 0.7]])
  fn = lambda means, covs, normals, viewdirs: torch.from_numpy(flat(means.cpu().numpy(), None).astype(F)).to(means.device)
  for lam in (0., 1e-3):
    baked = mesh.bake_texture(dm, color_fn=fn, cell=5, filter=0., sh_degree=2, sh_lambda=lam, return_float=True)
    want_sh, _, _ = S.bake(m, 5, DIRS[42], 2, lam, flat)
    assert np.array_equal(bits(baked['sh']), bits(want_sh))
    own = (baked['mask'] == 255).cpu().numpy()
    sh = baked['sh'].cpu().numpy()
    assert np.abs(sh[own][:, 1:]).max() < 1e-9 and not sh[~own].any()
    assert np.abs(sh[own][:, 0] * S.C0 - baked['texture_f32'].cpu().numpy()[own]).max() < 2e-7
    for view in range(len(VIEWS)):
      P, _ = projection(view, *SIZES[0])
      r = mesh.render_mesh(dm, None, None, *SIZES[0], texture=baked, proj=P, near=1e-3)
      f32 = mesh.render_mesh(dm, None, None, *SIZES[0], texture=dict(texture=baked['texture_f32'], uv=baked['uv']), proj=P, near=1e-3)
      assert torch.equal(r['face'], f32['face']) and float((r['rgb'] - f32['rgb']).abs().max()) <= BOUND


def test_defaults_change_nothing():
  """sh_degree=None returns the dict of the plain bake (the atlas restatement's, key for key); the SH bake's texture, mask and uv are the
  same bits; view_dependent=False and a dict without sh render the same image; two runs agree."""
  m = source('ico80')
  dm = to_device(m)
  fn = field_color_fn()
  plain = mesh.bake_texture(dm, color_fn=fn, cell=4, filter=0., return_float=True)
  assert sorted(plain) == ['layout', 'mask', 'texture', 'texture_f32', 'uv'] and sorted(mesh.bake_texture(dm, color_fn=fn, cell=4)) == ['layout', 'mask', 'texture', 'uv']
  s = A.samples(m, 4, 0.)
  lay = A.layout(80, 4)
  texture, mask, texture_f32 = A.store(lay, S.field_colour(s['means'], s['viewdirs']).astype(F), s['face'])
  assert plain['layout'] == lay and np.array_equal(plain['texture'].cpu().numpy(), texture) and np.array_equal(plain['mask'].cpu().numpy(), mask)
  assert np.array_equal(bits(plain['texture_f32']), bits(texture_f32)) and np.array_equal(bits(plain['uv']), bits(A.uvs(80, lay)))
  baked = mesh.bake_texture(dm, color_fn=fn, cell=4, filter=0., return_float=True, sh_degree=1, sh_dirs=DIRS[12])
  again = mesh.bake_texture(dm, color_fn=fn, cell=4, filter=0., return_float=True, sh_degree=1, sh_dirs=DIRS[12])
  assert sorted(baked) == sorted(list(plain) + ['sh', 'sh_degree', 'sh_dirs', 'sh_queries'])
  for k in ('texture', 'mask', 'texture_f32', 'uv'):
    assert torch.equal(baked[k], plain[k]), k
  assert torch.equal(baked['sh'].view(torch.int32), again['sh'].view(torch.int32)) and tuple(baked['sh'].shape) == (lay['H'], lay['W'], 4, 3)
  P, _ = projection(0, *SIZES[0])
  kw = dict(proj=P, near=1e-3, supersample=2)
  a = mesh.render_mesh(dm, None, None, *SIZES[0], texture=baked, view_dependent=False, **kw)
  b = mesh.render_mesh(dm, None, None, *SIZES[0], texture={k: baked[k] for k in ('texture', 'uv')}, **kw)
  c = mesh.render_mesh(dm, None, None, *SIZES[0], texture=baked, **kw)
  d = mesh.render_mesh(dm, None, None, *SIZES[0], texture=baked, **kw)
  for k in ('rgb', 'acc', 'face', 'depth', 'bary', 'normals'):
    assert torch.equal(a[k], b[k]) and torch.equal(c[k], d[k]), k
    assert (k == 'rgb') != torch.equal(a[k], c[k]), k
  assert tuple(c['rgb'].shape) == SIZES[0] + (3,) and tuple(c['face'].shape) == (2 * SIZES[0][0], 2 * SIZES[0][1])
  # the camera form finds the same eye as the projection form; an explicit origin is taken as given
  eye, target, focal = VIEWS[0]
  e = mesh.render_mesh(dm, R.pixtocam(focal, 48, 40), R.look_at(eye, target), *SIZES[0], texture=baked, near=1e-3, supersample=2)
  assert float((e['rgb'] - c['rgb']).abs().max()) < 1e-5
  g = mesh.render_mesh(dm, None, None, *SIZES[0], texture=baked, origin=(0., 0., 3.), **kw)
  assert not torch.equal(g['rgb'], c['rgb']) and torch.equal(g['face'], c['face'])


def test_chunk_sizes_give_the_same_sh():
  dm = to_device(source('ico80'))
  fn = field_color_fn()
  whole = mesh.bake_texture(dm, color_fn=fn, cell=3, filter=0., sh_degree=2, sh_dirs=DIRS[12])
  assert whole['layout']['n_samples'] == 480
  for chunk in (1, 7):
    part = mesh.bake_texture(dm, color_fn=fn, cell=3, filter=0., sh_degree=2, sh_dirs=DIRS[12], chunk=chunk)
    assert torch.equal(part['sh'].view(torch.int32), whole['sh'].view(torch.int32)) and part['sh_queries'] == whole['sh_queries'], chunk
    assert torch.equal(part['texture'], whole['texture'])


# ---- models

BINDS = ["Config.dataset_loader = 'procedural'", 'NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'NerfMLP.bottleneck_width = 128']
SEED = 20200823


def test_model_bake_and_file_round_trip(tmp_path):
  """A small Ref-NeRF model (view directions through the IDE) on the 80-face sphere at degree 1: finite, view-dependent, and the same
  image through a written and re-read PLY (float32 file; the float16 file to its rounding)."""
  from multinerf_amd import configs, models
  config = configs.load_preset('blender_refnerf', BINDS)
  model, _ = models.construct_model(SEED, None, config, device='cuda')
  assert model.nerf_plan.use_viewdirs
  m = source('ico80')
  dm = to_device(m)
  baked = mesh.bake_texture(dm, model=model, cell=4, chunk=2000, sh_degree=1)
  sh = baked['sh']
  assert bool(torch.isfinite(sh).all()) and tuple(sh.shape[2:]) == (4, 3) and 0 < baked['sh_queries'] <= 21 * int((baked['mask'] == 255).sum())
  assert float(sh[..., 1:, :].abs().max()) > 0               # the model's colour does depend on the direction
  P, _ = projection(0, *SIZES[0])
  r = mesh.render_mesh(dm, None, None, *SIZES[0], texture=baked, proj=P, near=1e-3)
  assert bool(torch.isfinite(r['rgb']).all())
  for sh_dtype, tol in (('float32', 0.), ('float16', 2. ** -11 * float(sh.abs().max()) * S.SUM_MAX_BASIS + 1e-6)):
    ply = str(tmp_path / f'{sh_dtype}.ply')
    mesh.write_ply(ply, m, texture=baked, sh_dtype=sh_dtype)
    back = mesh.read_ply(ply)
    from PIL import Image
    tex = dict(texture=np.array(Image.open(str(tmp_path / back['texture_file']))), uv=back['texcoord'], sh=back['texture_sh'])
    again = mesh.render_mesh(dm, None, None, *SIZES[0], texture=tex, proj=P, near=1e-3)
    assert float((again['rgb'] - r['rgb']).abs().max()) <= tol, sh_dtype


def test_model_without_view_directions():
  from multinerf_amd import configs, models
  config = configs.load_preset('blender_256', BINDS + ['Model.use_viewdirs = False'])
  model, _ = models.construct_model(SEED, None, config, device='cuda')
  assert not model.nerf_plan.use_viewdirs
  dm = to_device(source('ico80'))
  baked = mesh.bake_texture(dm, model=model, cell=4, chunk=2000, sh_degree=1, return_float=True)
  own = baked['mask'] == 255
  sh = baked['sh']
  scale = float(sh[own][:, 0].abs().max())
  assert bool(torch.isfinite(sh).all()) and float(sh[own][:, 1:].abs().max()) < 1e-9 * max(scale, 1.)
  assert float((sh[own][:, 0] * S.C0 - baked['texture_f32'][own]).abs().max()) <= 2e-7 * max(scale, 1.)


# ---- the scripts

def run(script, args):
  r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT),
                     timeout=300, cwd=ROOT)
  print(r.stdout[-3000:], r.stderr[-3000:])
  return r


def test_script_bakes_and_evaluates(tmp_path):
  from multinerf_amd import checkpoints, configs, models, train_utils
  binds = BINDS + ['Config.factor = 2']
  config = configs.load_preset('blender_refnerf', binds)
  model, variables = models.construct_model(SEED, None, config, device='cuda')
  field, _, _ = mesh.density_grid(lambda x, s: model.query_density(x[None], s)[0], (-1., -1., -1.), (1., 1., 1.), 9, chunk=2000)
  ck = str(tmp_path / 'ckpt')
  state, _ = train_utils.create_optimizer(config, variables)
  state.step = 7
  checkpoints.save_checkpoint(ck, model, state, 7)
  common = ['--preset', 'blender_refnerf']
  for b in binds + [f"Config.checkpoint_dir = '{ck}'"]:
    common += ['--gin_bindings', b]
  r = run('extract_mesh.py', common + ['--resolution', '9', '--bbox', '-1,-1,-1,1,1,1', '--density_threshold', repr(float(field.median())), '--chunk', '2000',
                                       '--texture', '4', '--texture_sh', '1'])
  assert r.returncode == 0
  out = os.path.join(ck, 'mesh')
  assert all(os.path.exists(os.path.join(out, n)) for n in ('mesh_step_7.ply', 'mesh_step_7.png', 'mesh_step_7_sh.npy'))
  line = [l for l in r.stdout.split('\n') if l.startswith('texture sh: ')]
  assert len(line) == 1 and line[0].startswith('texture sh: degree 1, 42 directions, ') and line[0].endswith(' colour queries')
  assert ', texture bake ' in r.stdout.split('seconds:')[1] and ' (sh ' in r.stdout.split('seconds:')[1]
  back = mesh.read_ply(os.path.join(out, 'mesh_step_7.ply'))
  stored = np.load(os.path.join(out, 'mesh_step_7_sh.npy'))
  assert stored.dtype == np.float16 and stored.shape[2:] == (4, 3) and back['texture_sh'].shape == stored.shape and np.isfinite(stored).all()
  assert 0 < int(line[0].split()[-3]) <= 21 * len(back['faces']) * 10      # 10 owned texels a face at cell 4, at most half of 42 directions each
  e = run('eval_mesh.py', common + ['--mesh', os.path.join(out, 'mesh_step_7.ply')])
  assert e.returncode == 0 and "view-dependent texture: spherical harmonics of degree 1, shaded at every pixel's view direction" in e.stdout
  a = open(os.path.join(out, 'mesh_eval', 'mesh_metric_psnr.txt')).read()
  e = run('eval_mesh.py', common + ['--mesh', os.path.join(out, 'mesh_step_7.ply'), '--no_view_dependent', '--out_dir', str(tmp_path / 'plain')])
  assert e.returncode == 0 and 'ignored (--no_view_dependent): the plain texture is scored' in e.stdout
  b = open(str(tmp_path / 'plain' / 'mesh_metric_psnr.txt')).read()
  assert len(a.split()) == len(b.split()) == 6 and a != b
  # a model that reads no view direction is refused in one line
  r = run('extract_mesh.py', ['--preset', 'blender_256', '--gin_bindings', 'Model.use_viewdirs = False', '--gin_bindings', f"Config.checkpoint_dir = '{ck}'",
                              '--texture', '4', '--texture_sh', '1'] + sum([['--gin_bindings', b] for b in BINDS], []))
  assert r.returncode != 0 and len([l for l in r.stderr.split('\n') if 'reads no view direction, nothing would change' in l]) == 1
