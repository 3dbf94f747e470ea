"""Texture atlas on the GPU (-m gpu): the kernels of csrc/atlas.hip through ops.atlas_samples / atlas_store / atlas_uvs and
mesh.bake_texture against the NumPy restatement (tests/atlas_ref.py), seam safety and linearity asserted on the kernels' own output,
bakes with an analytic colour function and with a small model, degenerate inputs, and extract_mesh.py --texture.
tests/test_atlas_cpu.py holds the preconditions (known answers of the restatement)."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multinerf_amd import mesh, ops
from tests import atlas_ref as A
from tests import mesh_clean_ref as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = (3, 4, 8, 13)
CHUNK = 1009                       # a prime: chunks split cells and waves


def to_device(m):
  return {k: torch.from_numpy(np.array(m[k])).cuda() for k in ('vertices', 'normals', 'faces')}


def bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def hand_mesh(T):
  """T faces over 3 T + 2 random vertices in [-1, 1]^3 with random (not unit) normals.  With T = 5: face 3 has zero normals at
  all three corners (the face normal takes over), face 4 has zero area and zero normals ((0, 0, 1) takes over)."""
  rng = np.random.default_rng(40 + T)
  V = 3 * T + 2
  verts, normals = rng.uniform(-1, 1, (V, 3)).astype(np.float32), rng.normal(size=(V, 3)).astype(np.float32)
  faces = np.stack([rng.permutation(V)[:3] for _ in range(T)]).astype(np.int32)
  if T == 5:
    faces[3], faces[4] = (9, 10, 11), (12, 13, 13)
    faces[:3] = np.where(faces[:3] >= 9, faces[:3] - 9, faces[:3])
    normals[9:14] = 0
  return dict(vertices=verts, normals=normals, faces=faces)


@functools.lru_cache(maxsize=None)
def source(name):
  m = dict(C.source_mesh('sphere')[0]) if name == 'sphere' else hand_mesh(int(name))
  m = {k: m[k] for k in ('vertices', 'normals', 'faces')}
  for a in m.values():
    a.setflags(write=False)
  return m


@functools.lru_cache(maxsize=None)
def restated(name, c):
  """The restatement's samples of a mesh (they do not depend on cols), computed once and shared."""
  s = A.samples(source(name), c)
  for a in s.values():
    a.setflags(write=False)
  return s


def kernel_samples(dm, lay, start=0, stop=None, **kw):
  out = ops.atlas_samples(dm, lay, start, lay['n_samples'] if stop is None else stop, **kw)
  assert [o.dtype for o in out] == [torch.float32] * 4 + [torch.int32]
  return dict(zip(('means', 'covs', 'normals', 'viewdirs', 'face'), (o.cpu().numpy() for o in out)))


# ---- against the restatement

CASES = [('1', None), ('2', None), ('5', 1), ('5', 2), ('sphere', None)]


@pytest.mark.parametrize('c', CELLS)
@pytest.mark.parametrize('name,cols', CASES)
def test_kernels_against_the_restatement(name, cols, c):
  m = source(name)
  T = len(m['faces'])
  dm = to_device(m)
  lay = ops.atlas_layout(T, c, cols)
  assert lay == A.layout(T, c, cols)
  want = restated(name, c)
  got = kernel_samples(dm, lay)
  n = lay['n_samples']
  assert [tuple(got[k].shape) for k in ('means', 'covs', 'normals', 'viewdirs', 'face')] == [(n, 3), (n, 3, 3), (n, 3), (n, 3), (n,)]
  assert np.array_equal(got['face'], want['face'])
  assert np.array_equal(bits(got['means']), bits(want['means'])) and np.array_equal(bits(got['covs']), bits(want['covs']))
  dn, dv = np.abs(got['normals'] - want['normals']).max(), np.abs(got['viewdirs'] - want['viewdirs']).max()
  same = np.array_equal(bits(got['normals']), bits(want['normals'])) and np.array_equal(bits(got['viewdirs']), bits(want['viewdirs']))
  print(f'{name} c {c} cols {lay["cols"]}: {lay["W"]} x {lay["H"]}, {n} samples, {int((got["face"] < 0).sum())} invalid, normals max |kernel - '
        f'numpy| {dn:.3e}, viewdirs {dv:.3e}, bit-equal {same}')
  assert dn <= 1e-6 and dv <= 1e-6
  assert all(np.isfinite(got[k]).all() for k in ('means', 'covs', 'normals', 'viewdirs'))
  invalid = got['face'] < 0
  assert invalid.sum() == (c * (c + 1) // 2 if T % 2 else 0)
  assert (got['means'][invalid] == 0).all() and (got['covs'][invalid] == 0).all()
  assert (got['normals'][invalid] == [0, 0, 1]).all() and (got['viewdirs'][invalid] == [0, 0, 1]).all()
  uv = ops.atlas_uvs(dm, lay)
  assert uv.dtype == torch.float32 and tuple(uv.shape) == (T, 3, 2)
  assert np.array_equal(bits(uv.cpu().numpy()), bits(A.uvs(T, lay)))
  # chunks of a prime number of samples, concatenated, are the one call, bit for bit
  parts = [kernel_samples(dm, lay, s, min(s + CHUNK, n)) for s in range(0, n, CHUNK)]
  for k in got:
    whole, cat = got[k], np.concatenate([p[k] for p in parts])
    assert np.array_equal(whole.view(np.uint32) if whole.dtype == np.float32 else whole, cat.view(np.uint32) if cat.dtype == np.float32 else cat), k


def test_fallback_normals_of_the_hand_mesh():
  """Face 3 of the 5-face mesh takes its face normal, face 4 (zero area) (0, 0, 1) with view direction (0, 0, 1)."""
  m = source('5')
  got = kernel_samples(to_device(m), ops.atlas_layout(5, 4))
  v = m['vertices'][m['faces'][3]].astype(np.float64)
  g = np.cross(v[1] - v[0], v[2] - v[0])
  g /= np.linalg.norm(g)
  assert np.abs(got['normals'][got['face'] == 3] - g).max() <= 1e-6 and np.abs(got['viewdirs'][got['face'] == 3] + g).max() <= 1e-6
  assert (got['face'] == 4).sum() == 10
  assert (got['normals'][got['face'] == 4] == [0, 0, 1]).all() and (got['viewdirs'][got['face'] == 4] == [0, 0, 1]).all()
  point = kernel_samples(to_device(m), ops.atlas_layout(5, 4), filter=0.)
  assert (point['covs'] == 0).all() and np.array_equal(bits(point['means']), bits(got['means']))


# ---- properties of the kernels' own output

def barycentric_points():
  """[32, 3]: the 3 corners, 3 points on each edge, 20 interior points (seeded).  All are multiples of 1 / 64: with the corners on
  texel centres every pixel position is a multiple of 1 / 64 of a texel."""
  corners = [(64, 0, 0), (0, 64, 0), (0, 0, 64)]
  edges = [p for t in (16, 32, 48) for p in ((64 - t, t, 0), (0, 64 - t, t), (t, 0, 64 - t))]
  rng = np.random.default_rng(7)
  interior = []
  while len(interior) < 20:
    i, j = rng.integers(1, 63, 2)
    if i + j <= 63:
      interior.append((int(i), int(j), int(64 - i - j)))
  return np.array(corners + edges + interior, np.float64) / 64.


def pixel_positions(uv, lay, bary):
  """[T, P, 2]: pixel positions (px, py from the top) of the barycentric points, from the kernel's corner UVs, float64."""
  uv = uv.astype(np.float64)
  corners = np.stack([uv[..., 0] * lay['W'], (1. - uv[..., 1]) * lay['H']], -1)                 # [T, 3, 2]
  return np.einsum('pk,tkd->tpd', bary, corners)


@pytest.mark.parametrize('name,cols,c', [('5', 2, 3), ('5', 1, 8), ('sphere', None, 4), ('sphere', None, 13)])
def test_seam_safety(name, cols, c):
  """One distinct colour per face (integers below 2^20, exact in float32 and float64) stored through the store kernel at the sample
  kernel's `face`; a bilinear lookup at 32 barycentric points of every face, through the UV kernel's corners, returns that
  face's colour EXACTLY: any non-zero weight on a neighbour's or an unowned texel (which holds 0) shows.

  The contract's argument is one in exact arithmetic.  A float32 UV is its exact value rounded, up to 2^-24 of itself, and the
  corners and edges of a chart lie exactly on the boundary between two texels' supports: rounding alone puts a weight of up to about
  2^-24 W on the texel beyond.  So the lookup positions are the kernel's UVs with that rounding removed: every exact position is a
  multiple of 1 / 64 texel (`barycentric_points`), the test asserts that the kernel's value is within float32 rounding of such a
  multiple (2^-22 max(W, H), three roundings: the quotient, 1 - v and the combination) and looks up at the multiple.  A half-texel error
  in either kernel is 32 of these steps and is not removed.  The raw float32 UVs are looked up as well: their colours may be off by
  the rounded-away weight times the colour range, and by no more.  Measured on the MI355X with the raw UVs (colours up to 2^20):
  the sphere at c = 4 (325 x 320) 49,475 of 331,648 lookups not exact, largest colour error 7.6; at c = 13 (980 x 975) 54,300 and
  0.042; the 5-face meshes 5 and 7 of 160, 3e-6 and 1e-5.  The positions sat within 9.7e-6 and 4.3e-5 texels of their grid."""
  m = source(name)
  T = len(m['faces'])
  dm = to_device(m)
  lay = ops.atlas_layout(T, c, cols)
  H, W, n = lay['H'], lay['W'], lay['n_samples']
  face = ops.atlas_samples(dm, lay, 0, n)[4]
  colour = np.stack([np.arange(T) + 1, 2 ** 20 - 1 - np.arange(T), (7 * np.arange(T) + 3) % 2 ** 20], -1).astype(np.float32)
  rgb = torch.from_numpy(np.concatenate([colour, np.zeros((1, 3), np.float32)])[face.cpu().numpy()]).cuda()     # face -1: the last row
  atlas, mask = torch.zeros((H, W, 3), dtype=torch.uint8).cuda(), torch.zeros((H, W), dtype=torch.uint8).cuda()
  atlas_f32 = torch.zeros((H, W, 3), dtype=torch.float32).cuda()
  ops.atlas_store(dm, lay, 0, rgb, face, atlas, mask, atlas_f32)
  image = atlas_f32.cpu().numpy().astype(np.float64)
  uv = ops.atlas_uvs(dm, lay).cpu().numpy()
  bary = barycentric_points()
  pos = pixel_positions(uv, lay, bary)
  snapped = np.round(pos * 64.) / 64.
  off = np.abs(pos - snapped).max()
  got = A.sample_bilinear_px(image, snapped[..., 0], snapped[..., 1])                          # [T, 32, 3]
  raw = A.sample_bilinear(image, np.einsum('pk,tkd->tpd', bary, uv.astype(np.float64)))
  leak = np.abs(raw - colour[:, None, :].astype(np.float64)).max()
  print(f'{name} c {c}: {W} x {H}; positions off their 1/64 grid by at most {off:.3e} texels (bound {2. ** -22 * max(W, H):.3e}); raw float32 '
        f'UVs: max |colour error| {leak:.3e} (bound {2. ** -22 * max(W, H) * 2 ** 21:.3e}), {int((raw != colour[:, None, :]).any(-1).sum())} of '
        f'{T * 32} lookups not exact')
  assert off <= 2. ** -22 * max(W, H)
  assert np.array_equal(got, np.broadcast_to(colour[:, None, :].astype(np.float64), got.shape))
  assert leak <= 2. ** -22 * max(W, H) * 2 ** 21             # two axes, a colour difference below 2^20 each
  assert np.array_equal(mask.cpu().numpy() == 255, A.scatter(lay, np.ones(n), face.cpu().numpy()) == 1)


@pytest.mark.parametrize('c', (3, 8))
def test_linearity(c):
  """An atlas holding A p + b (float64) at the kernel's sample positions p returns A (sum b_i v_i) + b at the UV of the barycentric
  point b, to 1e-5: float32 rounding of the positions times |A| <= 1, with |p| <= 1.  A half-texel error in either mapping would
  show as about |A| |edge| / (2 (c - 2)), two to three orders above the bound.

  That budget holds the rounding of the POSITIONS.  The rounding of the float32 UVs is a second term, and on the boundary of a
  chart it is not multiplied by the chart's own gradient but by the jump to the neighbouring chart (`test_seam_safety`): up to 2^-22
  max(W, H) texels times the range of the image, which on this atlas is above 1e-5 (measured with the raw UVs: 1.3e-5 at c = 3,
  2.6e-5 at c = 8).  So the 1e-5 is asserted at the UVs with their rounding removed, as in `test_seam_safety` (positions are
  multiples of 1 / 64 texel), and the raw UVs are held to 1e-5 plus that second term."""
  m = dict(source('sphere'))
  m['vertices'] = (m['vertices'] / np.float32(0.75)).astype(np.float32)                      # the sphere of radius 0.6: |p| <= 0.8
  assert np.linalg.norm(m['vertices'], axis=1).max() <= 1.
  T = len(m['faces'])
  dm = to_device(m)
  lay = ops.atlas_layout(T, c)
  s = kernel_samples(dm, lay)
  rng = np.random.default_rng(3)
  M = rng.normal(size=(3, 3))
  M /= np.linalg.norm(M, 2)
  b = rng.uniform(-1, 1, 3)
  image = A.scatter(lay, s['means'].astype(np.float64) @ M.T + b, s['face'])
  uv = ops.atlas_uvs(dm, lay).cpu().numpy()
  bary = barycentric_points()
  pos = pixel_positions(uv, lay, bary)
  snapped = np.round(pos * 64.) / 64.
  side = max(lay['W'], lay['H'])
  assert np.abs(pos - snapped).max() <= 2. ** -22 * side
  want = np.einsum('pk,tkd->tpd', bary, m['vertices'][m['faces']].astype(np.float64)) @ M.T + b
  err = np.abs(A.sample_bilinear_px(image, snapped[..., 0], snapped[..., 1]) - want).max()
  raw = np.abs(A.sample_bilinear(image, np.einsum('pk,tkd->tpd', bary, uv.astype(np.float64))) - want).max()
  edge = np.linalg.norm(m['vertices'][m['faces'][:, 1]] - m['vertices'][m['faces'][:, 0]], axis=1).mean()
  jump = (image.max((0, 1)) - image.min((0, 1))).max()
  print(f'linearity c {c}: max |lookup - (A p + b)| {err:.3e} (raw float32 UVs {raw:.3e}, their bound {1e-5 + 2. ** -22 * side * jump:.3e}); '
        f'a half-texel error would be about {edge / (2 * (c - 2)):.3e}')
  assert err <= 1e-5
  assert raw <= 1e-5 + 2. ** -22 * side * jump


# ---- bake_texture with an analytic colour function

def analytic_color(means, covs, normals, viewdirs):
  """A fixed smooth function of mean and view direction that leaves [0, 1] in places; products and sums only, each correctly rounded,
  so equal inputs give equal bits whatever the device and the chunking."""
  return 0.5 + 0.9 * (means * means.roll(1, -1)) - 0.7 * viewdirs + 0.4 * (viewdirs * means)


def restated_bake(name, c, cols=None):
  m = source(name)
  lay = A.layout(len(m['faces']), c, cols)
  s = restated(name, c)
  rgb = analytic_color(*(torch.from_numpy(np.array(s[k])).cuda() for k in ('means', 'covs', 'normals', 'viewdirs')))
  return lay, A.store(lay, rgb.cpu().numpy(), s['face']), s


@pytest.mark.parametrize('name,cols,c', [('1', None, 3), ('5', 2, 4), ('sphere', None, 4), ('sphere', None, 8)])
def test_bake_with_an_analytic_color_fn(name, cols, c):
  dm = to_device(source(name))
  lay, (texture, mask, texture_f32), s = restated_bake(name, c, cols)
  out = mesh.bake_texture(dm, color_fn=analytic_color, cell=c, cols=cols, return_float=True)
  assert sorted(out) == ['layout', 'mask', 'texture', 'texture_f32', 'uv'] and out['layout'] == lay
  assert out['texture'].dtype == torch.uint8 and out['mask'].dtype == torch.uint8 and out['texture_f32'].dtype == torch.float32
  assert np.array_equal(out['texture'].cpu().numpy(), texture) and np.array_equal(out['mask'].cpu().numpy(), mask)
  assert np.array_equal(bits(out['texture_f32'].cpu().numpy()), bits(texture_f32))
  assert np.array_equal(out['mask'].cpu().numpy() == 255, A.scatter(lay, np.ones(lay['n_samples']), s['face']) == 1)
  assert set(np.unique(out['mask'].cpu().numpy())) <= {0, 255} and texture.min() == 0 and texture.max() == 255     # the clip is exercised
  assert np.array_equal(bits(out['uv'].cpu().numpy()), bits(A.uvs(len(source(name)['faces']), lay)))
  chunked = mesh.bake_texture(dm, color_fn=analytic_color, cell=c, cols=cols, return_float=True, chunk=CHUNK)
  for k in ('texture', 'mask', 'texture_f32', 'uv'):
    assert torch.equal(chunked[k], out[k]), k
  plain = mesh.bake_texture(dm, color_fn=analytic_color, cell=c, cols=cols)
  assert sorted(plain) == ['layout', 'mask', 'texture', 'uv'] and torch.equal(plain['texture'], out['texture'])


# ---- degenerate inputs

def test_degenerate_inputs():
  empty = dict(vertices=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32))
  out = mesh.bake_texture(to_device(empty), color_fn=analytic_color, cell=8, return_float=True)
  assert [tuple(out[k].shape) for k in ('texture', 'mask', 'uv', 'texture_f32')] == [(0, 0, 3), (0, 0), (0, 3, 2), (0, 0, 3)]
  assert out['layout']['n_samples'] == 0
  orphan = dict(empty, vertices=np.zeros((4, 3), np.float32), normals=np.zeros((4, 3), np.float32))          # vertices, no faces
  assert tuple(mesh.bake_texture(to_device(orphan), color_fn=analytic_color)['texture'].shape) == (0, 0, 3)

  m = {k: np.array(v) for k, v in source('5').items()}
  m['faces'][:3] = ((14, 15, 16), (3, 4, 5), (0, 0, 0))      # no vertex shared; face 2 has zero area and a normal: a point
  m['vertices'][5, 1] = np.nan                                # face 1 has a NaN vertex
  dm = to_device(m)
  lay = ops.atlas_layout(5, 4)
  s = kernel_samples(dm, lay)
  assert all(np.isfinite(s[k]).all() for k in ('means', 'covs', 'normals', 'viewdirs'))
  assert not (s['face'] == 1).any() and (s['face'] == -1).sum() == 10 + 10 and all((s['face'] == f).sum() == 10 for f in (0, 2, 3, 4))
  bad = s['face'].reshape(3, 4, 5)[0] == -1
  assert np.array_equal(bad, np.array(A.samples(source('2'), 4)['face']).reshape(4, 5) == 1)    # exactly the upper half of cell 0
  assert np.abs(s['means'][s['face'] == 2] - m['vertices'][0]).max() <= 1e-6 and (s['covs'][s['face'] == 2] == 0).all()
  out = mesh.bake_texture(dm, color_fn=analytic_color, cell=4, return_float=True)
  assert torch.isfinite(out['texture_f32']).all()
  assert np.array_equal(out['mask'].cpu().numpy() == 255, A.scatter(lay, np.ones(lay['n_samples']), s['face']) == 1)
  assert (out['texture'].cpu().numpy()[out['mask'].cpu().numpy() == 0] == 0).all()

  for index in (-1, 17):
    broken = dict(m, faces=np.array([[0, 1, 2], [3, index, 4]], np.int32))
    with pytest.raises(ValueError):
      mesh.bake_texture(to_device(broken), color_fn=analytic_color)
    with pytest.raises(ValueError):
      ops.atlas_samples(to_device(broken), ops.atlas_layout(2, 4), 0, 20)
  good = to_device(source('5'))
  with pytest.raises(ValueError):
    mesh.bake_texture(good, color_fn=analytic_color, cell=2)
  with pytest.raises(ValueError):
    ops.atlas_layout(5, 2)
  with pytest.raises(ValueError):
    mesh.bake_texture(good)
  with pytest.raises(ValueError):
    mesh.bake_texture(good, color_fn=analytic_color, model=object())
  with pytest.raises(ValueError):
    ops.atlas_samples(good, ops.atlas_layout(5, 4), 0, 61)                            # beyond the 60 samples
  with pytest.raises(ValueError):
    ops.atlas_samples(good, dict(ops.atlas_layout(5, 4), W=11), 0, 60)                # not the contract's layout
  with pytest.raises(ValueError):
    ops.atlas_samples(good, ops.atlas_layout(5, 4), 0, 60, filter=float('nan'))


# ---- a small model (the one of tests/test_gpu_mesh.py), its mesh simplified by 2 grid spacings

@pytest.fixture(scope='module')
def model_case():
  from multinerf_amd import configs, models
  from tests.test_gpu_mesh import BINDS, BOX, CHUNK as MLP_CHUNK, RES, SEED, STD
  config = configs.load_preset('blender_256', BINDS)
  model, variables = models.construct_model(SEED, None, config, device='cuda')
  field, _, spacing = mesh.density_grid(lambda x, s: model.query_density(x[None], s)[0], *BOX, RES, std=STD, chunk=MLP_CHUNK)
  threshold = float(field.median())
  full = mesh.extract_mesh(model, *BOX, RES, threshold, std=STD, chunk=MLP_CHUNK)
  small = mesh.simplify(full, 2. * spacing)
  return dict(config=config, model=model, variables=variables, threshold=threshold, spacing=spacing, full=full, small=small, chunk=MLP_CHUNK)


def test_model_bake_is_the_mlp_on_the_samples(model_case):
  model, m, chunk = model_case['model'], model_case['small'], model_case['chunk']
  T = int(m['faces'].shape[0])
  assert T > 0
  out = mesh.bake_texture(m, model=model, cell=4, chunk=chunk, return_float=True)
  lay = out['layout']
  plan = model.nerf_plan
  rgbs, faces = [], []
  for start in range(0, lay['n_samples'], chunk):
    stop = min(start + chunk, lay['n_samples'])
    means, covs, _, viewdirs, face = ops.atlas_samples(m, lay, start, stop)
    glo = torch.zeros((stop - start, plan.glo), dtype=torch.float32, device=means.device) if plan.glo > 0 else None
    rgb = model.nerf_hp(None, (means[:, None], covs[:, None]), viewdirs=viewdirs if plan.use_viewdirs else None, glo_vec=glo)['rgb']
    rgbs.append(rgb.reshape(stop - start, 3).to(torch.float32))
    faces.append(face)
  rgb, face = torch.cat(rgbs), torch.cat(faces).cpu().numpy()
  quantised = torch.floor(torch.clamp(rgb, 0., 1.) * 255. + 0.5).to(torch.uint8).cpu().numpy()
  texture, mask, texture_f32 = A.store(lay, rgb.cpu().numpy(), face)
  own = mask == 255
  print(f'model bake: T {T}, {lay["W"]} x {lay["H"]}, {lay["n_samples"]} samples in chunks of {chunk}, rgb {float(rgb.min()):.3f} .. {float(rgb.max()):.3f}')
  assert torch.isfinite(out['texture_f32']).all() and np.isfinite(rgb.cpu().numpy()).all()
  assert np.array_equal(out['mask'].cpu().numpy(), mask) and np.array_equal(bits(out['texture_f32'].cpu().numpy()), bits(texture_f32))
  assert np.array_equal(out['texture'].cpu().numpy(), texture)
  assert np.array_equal(out['texture'].cpu().numpy()[own], A.scatter(lay, quantised, face)[own])         # torch's quantisation, too
  again = mesh.bake_texture(m, model=model, cell=4, chunk=chunk, return_float=True)
  for k in ('texture', 'mask', 'texture_f32', 'uv'):
    assert torch.equal(again[k], out[k]), k


# ---- the script

def run_script(model_case, tmp_path, extra):
  from multinerf_amd import checkpoints, train_utils
  from tests.test_gpu_mesh import BINDS, RES, STD
  ck = str(tmp_path / 'ckpt')
  if not os.path.exists(ck):
    state, _ = train_utils.create_optimizer(model_case['config'], model_case['variables'])
    state.step = 7
    checkpoints.save_checkpoint(ck, model_case['model'], state, 7)
  args = ['--preset', 'blender_256']
  for b in BINDS + [f"Config.checkpoint_dir = '{ck}'"]:
    args += ['--gin_bindings', b]
  args += ['--resolution', str(RES), '--bbox', '-1,-1,-1,1,1,1', '--density_threshold', repr(model_case['threshold']), '--std', str(STD),
           '--chunk', str(model_case['chunk']), '--simplify', '2', '--texture', '4'] + extra
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'extract_mesh.py')] + args, capture_output=True, text=True,
                     env=dict(os.environ, PYTHONPATH=ROOT), timeout=300, cwd=ROOT)
  print(r.stdout[-2000:], r.stderr[-2000:])
  assert r.returncode == 0
  return ck, r.stdout


def test_script_writes_the_texture(model_case, tmp_path):
  from PIL import Image
  want = mesh.bake_texture(model_case['small'], model=model_case['model'], cell=4, chunk=model_case['chunk'])
  lay = want['layout']
  ck, stdout = run_script(model_case, tmp_path, [])
  back = mesh.read_ply(os.path.join(ck, 'mesh', 'mesh_step_7.ply'))
  assert np.array_equal(back['faces'], model_case['small']['faces'].cpu().numpy())
  assert np.array_equal(bits(back['texcoord']), bits(want['uv'].cpu().numpy())) and back['texture_file'] == 'mesh_step_7.png'
  assert np.array_equal(np.asarray(Image.open(os.path.join(ck, 'mesh', 'mesh_step_7.png'))), want['texture'].cpu().numpy())
  assert f'texture: {lay["W"]} x {lay["H"]}, {lay["n_samples"]} samples, cell 4' in stdout
  assert ', texture bake ' in stdout.split('seconds:')[1]


def test_script_writes_an_obj(model_case, tmp_path):
  from PIL import Image
  out = str(tmp_path / 'm.obj')
  _, stdout = run_script(model_case, tmp_path, ['--out', out])
  small = model_case['small']
  V, T = int(small['vertices'].shape[0]), int(small['faces'].shape[0])
  assert all(os.path.exists(str(tmp_path / n)) for n in ('m.obj', 'm.mtl', 'm.png'))
  kinds = [l.split(' ')[0] for l in open(out).read().split('\n') if l]
  assert (kinds.count('v'), kinds.count('vn'), kinds.count('vt'), kinds.count('f')) == (V, V, 3 * T, T)
  assert 'map_Kd m.png' in open(str(tmp_path / 'm.mtl')).read()
  lay = ops.atlas_layout(T, 4)
  assert np.asarray(Image.open(str(tmp_path / 'm.png'))).shape == (lay['H'], lay['W'], 3) and 'texture: ' in stdout
