"""Render paths on the GPU (-m gpu): the visualisation kernels (mnr_weighted_percentile, mnr_vis_cmap, mnr_vis_matte) and
mnr_spherical_rays against the reference's recorded outputs (tests/golden/render_path.npz, made by
tests/golden/make_golden_render.py) and the float64 restatements of tests/render_ref.py (which tests/test_render_cpu.py
holds to those records); multinerf_amd.vis composed; the dataset with Config.render_path on the device; render.py end to end.

Bounds.
  * Weighted percentile: 1 float32 ulp of the float64 result (the kernel sums in float64 and rounds once; the fixtures'
    weights are 0 or >= 1e-3, so the interpolation weight (T - acc[j]) / (acc[j+1] - acc[j]) is conditioned to 1e-10; the
    case with ties has weights that are multiples of 1/1024, whose sums are exact in any order).  Two runs: bit-equal.
  * Colour map: every pixel is exactly an entry of the float32 table, at most one entry from the float64 one, and off it in
    at most 0.5 % of the pixels (the reference's own arithmetic in float32 gives 0 of 3072 on such inputs).  Three
    channels without a table: 5e-7 (a division and a clip in float32 is what is allowed for; the kernel rounds once).
  * Matte: 5e-7 (two products and a sum of values in [0, 1]).
  * Composed (percentile + colour map + matte) against the reference: 5e-7, except in at most 0.5 % of the pixels, where
    the largest step between adjacent table entries is allowed on top.
  * Ray panels: float32 resampling against the float64 record has no bound that can be derived; RAY_PANEL_BOUND is ten
    times the largest difference measured on the MI355X (profiles/render_path.md).
  * Spherical rays: 1 float32 ulp.
The figures are printed before they are asserted.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import camera_utils, checkpoints, configs, datasets, ops, train_utils, utils, vis
from tests import render_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'render_path.npz')

PIX_BOUND = 5e-7
LUT_SHARE = 0.005
RAY_PANEL_BOUND = {'ray_colors': 10 * 5.12e-5, 'ray_weights': 10 * 3.93e-3}      # 10 x measured (profiles/render_path.md)


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')


@pytest.fixture(scope='module')
def g():
  return np.load(GOLDEN)


def _dev(x, dtype=torch.float32):
  return torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float64)), dtype=dtype).cuda()


def _np(t):
  return t.cpu().numpy().astype(np.float64)


def _f32(x):
  return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- mnr_weighted_percentile


def _check_percentiles(x, w, ps, golden=None, tag=''):
  dx, dw = _dev(x), _dev(w)
  got, again = [], []
  for k in range(0, len(ps), 4):                                                 # the entry takes up to 4 at once
    got.append(ops.weighted_percentile(dx, dw, list(ps[k:k + 4])))
    again.append(ops.weighted_percentile(dx, dw, list(ps[k:k + 4])))
  torch.cuda.synchronize()
  got, again = torch.cat(got), torch.cat(again)
  assert got.dtype == torch.float32 and got.shape == (len(ps),)
  want = ref.weighted_percentile(x, w, ps)
  out = _np(got)
  for p, a, b in zip(ps, out, want):
    print(f'{tag} p = {p}: kernel {a:.9g} float64 {b:.17g} diff {abs(a - b):.3g} (1 ulp = {float(ref.ulp32(b)):.3g})')
  assert (np.abs(out - want) <= ref.ulp32(want)).all()
  if golden is not None:
    assert (np.abs(out - golden) <= ref.ulp32(golden)).all()
  assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()            # bit for bit
  return out


@pytest.mark.parametrize('tag', ['wp_a', 'wp_b', 'wp_triplet', 'wp_tied', 'wp_zero'])
def test_weighted_percentile_kernel_equals_the_reference(g, tag):
  """37 x 53 (1961 values: two workgroups, no multiple of 64 or 1024), 3 x 5, the triplet (N = 3 NW: the clamp), ties with
  zero weights in front and at the end at p in {0, 0.5, 50, 99.5, 100}, all-zero weights."""
  x, w, ps = g[f'{tag}/x'], g[f'{tag}/w'], g[f'{tag}/ps']
  out = _check_percentiles(x, w, ps, g[f'{tag}/out'], tag)
  if tag == 'wp_zero':
    assert (out == x.max()).all()
  if tag == 'wp_triplet':
    assert x.size == 3 * w.size


def test_weighted_percentile_kernel_large(g):
  """More values than 1024 segments of 1024: every thread sums a chunk of 5 (the other launch shape); the weighted median of
  equal weights is the plain one; already-sorted input is taken as given."""
  rs = np.random.RandomState(5)
  n = 1024 * 1024 + 777
  x = _f32(rs.uniform(2, 6, n))
  w = _f32(np.where(rs.uniform(size=n) < 0.1, 0.0, rs.uniform(1e-3, 1, n)))
  _check_percentiles(x, w, [0.5, 50., 99.5], tag='large')
  xs = np.sort(x)
  got = _np(ops.weighted_percentile(_dev(xs), torch.ones(n).cuda(), [50.], assume_sorted=True))
  want = ref.weighted_percentile(xs, np.ones(n), [50.])
  assert abs(got[0] - want[0]) <= ref.ulp32(want[0])


def test_vis_argument_errors_are_raised_not_launched():
  x = torch.zeros((6, 7)).cuda()
  with pytest.raises(ValueError, match='1 to 4 are taken at once'):
    ops.weighted_percentile(x, x, [1., 2., 3., 4., 5.])
  with pytest.raises(ValueError, match=r'percentile 101 is outside \[0, 100\]'):
    ops.weighted_percentile(x, x, [101.])
  with pytest.raises(ValueError, match='float32'):
    ops.weighted_percentile(x.double(), x, [50.])
  lohi = torch.tensor([0., 1.]).cuda()
  lut = torch.zeros((4, 3)).cuda()
  with pytest.raises(ValueError, match='a colour map takes a 1-channel value'):
    ops.vis_cmap(torch.zeros((6, 7, 3)).cuda(), lohi, lut=lut)
  with pytest.raises(ValueError, match='no colour map a 3-channel value'):
    ops.vis_cmap(x, lohi)
  with pytest.raises(ValueError, match='needs lo / hi'):
    ops.vis_cmap(x, None, lut=lut)
  with pytest.raises(ValueError, match='unknown curve'):
    ops.vis_cmap(x, lohi, lut=lut, curve='sqrt')
  with pytest.raises(ValueError, match=r'acc \(6, 6\) must be \[6,7\]'):
    ops.vis_cmap(x, lohi, lut=lut, acc=torch.zeros((6, 6)).cuda())
  with pytest.raises(ValueError, match='checker width 0 must be positive'):
    ops.vis_matte(torch.zeros((6, 7, 3)).cuda(), x, width=0)
  with pytest.raises(ValueError, match='unknown pre-op'):
    ops.vis_matte(torch.zeros((6, 7, 3)).cuda(), x, preop='exp')
  with pytest.raises(ValueError, match='directions and distance go together'):
    ops.vis_matte(None, x, preop='coord_mod', origins=torch.zeros((6, 7, 3)).cuda(), distance=x)
  with pytest.raises(ValueError, match='curve_fn must be one of'):
    vis.visualize_cmap(x, x, lut, curve_fn=torch.log)


# ----------------------------------------------------------------------------- mnr_vis_cmap


def _lut_offsets(got, lut32, idx_ref):
  """Per pixel the d in {-1, 0, 1} with got == lut32[idx_ref + d] exactly (2 where there is none)."""
  n = len(lut32)
  d = np.full(idx_ref.shape, 2)
  for cand in (1, -1, 0):
    k = np.clip(idx_ref + cand, 0, n - 1)
    d = np.where((got == lut32[k]).all(-1), cand, d)
  return d


def test_vis_cmap_kernel_picks_the_table_entries(g):
  lut = g['lut/turbo']
  lut32 = lut.astype(np.float32)
  d_lut, value = _dev(lut), g['cmap/value']
  cases = [('percentile bounds, -log', _f32(g['cmap/lohi'] + [-ref.F32_EPS, ref.F32_EPS]), 'neg_log', None),
           ('explicit lo / hi', np.array([2.5, 5.0]), 'neg_log', None),
           ('hi < lo, log(x)', np.array([5.5, 2.25]), 'ln', None),
           ('modulus', np.array([0., 1.]), None, 0.25)]
  for name, lohi, curve, modulus in cases:
    u8 = torch.zeros((37, 53, 3), dtype=torch.uint8).cuda()
    got = ops.vis_cmap(_dev(value), _dev(lohi), curve=curve, modulus=modulus, lut=d_lut, out_u8=u8).cpu().numpy()
    _, idx = ref.visualize_cmap_pixels(value, lohi[0], lohi[1], curve, modulus=modulus, lut=lut)
    d = _lut_offsets(got, lut32, idx)
    share = float((d != 0).mean())
    print(f'{name}: entries off the float64 index in {int((d != 0).sum())} of {d.size} pixels, {len(np.unique(idx))} entries in use')
    assert got.shape == (37, 53, 3) and (np.abs(d) <= 1).all()
    assert share <= LUT_SHARE
    assert len(np.unique(idx)) > 100                                             # (the case spreads over the table)
    assert np.array_equal(u8.cpu().numpy(), (np.clip(got.astype(np.float64), 0, 1) * 255.).astype(np.uint8))
  # only the 8-bit image
  only = ops.vis_cmap(_dev(value), _dev(cases[1][1]), curve='neg_log', lut=d_lut, out_u8=u8, want_f32=False)
  assert only is u8


def test_vis_cmap_kernel_three_channels_nan_and_matte(g):
  value3, weight = g['cmap/value3'], g['cmap/weight']
  lohi = _f32(g['cmap/lohi3'] + [-ref.F32_EPS, ref.F32_EPS])
  got = _np(ops.vis_cmap(_dev(value3), _dev(lohi), curve='log'))
  want, _ = ref.visualize_cmap_pixels(value3, lohi[0], lohi[1], 'log')
  print(f'three channels: max diff {np.abs(got - want).max():.3g}; clipped at 0: {(want == 0).sum()}, at 1: {(want == 1).sum()}')
  assert np.abs(got - want).max() <= PIX_BOUND and (want == 0).any() and (want == 1).any()
  got = _np(ops.vis_cmap(_dev(value3), _dev(lohi), curve='log', acc=_dev(weight), dark=0.3, light=0.9, width=3))
  want, _ = ref.visualize_cmap_pixels(value3, lohi[0], lohi[1], 'log', acc=weight, dark=0.3, light=0.9, width=3)
  assert np.abs(got - want).max() <= PIX_BOUND
  # NaN and infinities: nan_to_num(clip(.)) puts NaN into entry 0
  lut = g['lut/turbo']
  v = g['cmap/value'].copy()
  v[0, 0], v[5, 7], v[36, 52], v[1, 1] = np.nan, np.inf, -np.inf, 0.0
  got = ops.vis_cmap(_dev(v), _dev(np.array([2.5, 5.0])), lut=_dev(lut)).cpu().numpy()
  lut32 = lut.astype(np.float32)
  assert (got[0, 0] == lut32[0]).all() and (got[5, 7] == lut32[-1]).all() and (got[36, 52] == lut32[0]).all() and (got[1, 1] == lut32[0]).all()
  got = ops.vis_cmap(_dev(v), _dev(np.array([2.5, 5.0])), lut=_dev(lut), curve='neg_log').cpu().numpy()
  assert (got[0, 0] == lut32[0]).all() and (got[1, 1] == lut32[-1]).all()       # -log(0 + eps) is the largest value


# ----------------------------------------------------------------------------- mnr_vis_matte


@pytest.mark.parametrize('width', [8, 3])
def test_vis_matte_kernel_every_preop(g, width):
  rs = np.random.RandomState(width)
  H, W = 37, 53
  acc = _f32(np.clip(rs.uniform(-0.2, 1.2, (H, W)), 0, 1))
  x3, x1 = _f32(rs.uniform(0, 1, (H, W, 3))), _f32(rs.normal(size=(H, W, 1)) * 2)
  o, d, t = _f32(rs.normal(size=(H, W, 3)) * 3), _f32(rs.normal(size=(H, W, 3))), _f32(rs.uniform(0.5, 6, (H, W)))
  kw = dict(dark=0.8, light=1.0, width=width) if width == 8 else dict(dark=0.25, light=0.6, width=width)
  cases = [(None, x3, {}), ('half', _f32(2 * x3 - 1), {}), ('tanh', x1, {}),
           ('coord_mod', None, dict(origins=o, directions=d, distance=t)), ('coord_mod', None, dict(origins=o))]
  for name, x, extra in cases:
    got = _np(ops.vis_matte(None if x is None else _dev(x), _dev(acc), preop=name, **{k: _dev(v) for k, v in extra.items()}, **kw))
    want = ref.matte(ref.preop(name, x, **extra), acc, **kw)
    print(f'width {width} pre-op {name}: max diff {np.abs(got - want).max():.3g}')
    assert got.shape == want.shape and np.abs(got - want).max() <= PIX_BOUND
  bg = ref.checker(H, W, **kw)
  assert len(np.unique(bg)) == 2 and bg[0, 0] == kw['dark'] and bg[0, width] == kw['light'] and bg[width, width] == kw['dark']
  got = _np(vis.matte(_dev(x3), _dev(acc)))                                       # the public wrapper, its defaults
  assert np.abs(got - ref.matte(x3, acc)).max() <= PIX_BOUND


# ----------------------------------------------------------------------------- composed


def _check_lut_image(name, got, want, lut):
  """Two tolerances: 5e-7, and in at most 0.5 % of the pixels the largest step between adjacent table entries on top."""
  step = float(np.abs(np.diff(lut, axis=0)).max())
  diff = np.abs(got - want).max(-1)
  off = diff > PIX_BOUND
  print(f'{name}: {int(off.sum())} of {off.size} pixels off by more than {PIX_BOUND} (largest {diff.max():.3g}, table step {step:.3g}), '
        f'the others at most {diff[~off].max():.3g}')
  assert got.shape == want.shape
  assert float(off.mean()) <= LUT_SHARE
  assert (diff[off] <= step + PIX_BOUND).all()


def test_visualize_cmap_composed_equals_the_reference(g):
  value, weight, turbo = _dev(g['cmap/value']), _dev(g['cmap/weight']), _dev(g['lut/turbo'])
  got = _np(vis.visualize_cmap(value, weight, turbo, curve_fn=vis.CURVE_NEG_LOG))
  _check_lut_image('percentile + turbo + matte', got, g['cmap/out'], g['lut/turbo'])
  got = _np(vis.visualize_cmap(value, weight, g['lut/turbo'], lo=2.5, hi=5.0, curve_fn='neg_log', matte_background=False))
  _check_lut_image('explicit bounds, no matte', got, g['cmap/out_lohi'], g['lut/turbo'])
  got = _np(vis.visualize_cmap(value, weight, turbo, modulus=0.25))
  _check_lut_image('modulus', got, g['cmap/out_mod'], g['lut/turbo'])
  got = _np(vis.visualize_cmap(_dev(g['cmap/value3']), weight, None, curve_fn=vis.CURVE_LOG))
  print(f'three channels: max diff {np.abs(got - g["cmap/out_c3"]).max():.3g}')
  assert np.abs(got - g['cmap/out_c3']).max() <= PIX_BOUND
  lohi = _np(vis.weighted_percentile(value, weight, [0.5, 99.5]))
  assert (np.abs(lohi - g['cmap/lohi']) <= ref.ulp32(g['cmap/lohi'])).all()
  with pytest.raises(ValueError, match='value must have 3 channels'):
    vis.visualize_cmap(value[..., None], weight, None)
  h = torch.linspace(0, 1, 7).cuda()
  want = np.stack([np.sin(np.pi * (k / 6 - _np(h)))**2 for k in (3, 5, 7)], -1)
  assert np.abs(_np(vis.sinebow(h)) - want).max() <= 1e-6


def _suite_inputs(g):
  rendering = {}
  for k in g.files:
    if not k.startswith('suite/in/'):
      continue
    parts = k.split('/')[2:]
    if len(parts) == 2:
      rendering.setdefault(parts[0], {})[int(parts[1])] = _dev(g[k])
    else:
      rendering[parts[0]] = _dev(g[k])
  for k, v in rendering.items():
    if isinstance(v, dict):
      rendering[k] = [v[i] for i in range(len(v))]
  rays = utils.Rays(origins=rendering.pop('origins'), directions=rendering.pop('directions'), viewdirs=None, radii=None,
                    imageplane=None, lossmult=None, near=None, far=None, cam_idx=None)
  return rendering, rays


def test_visualize_suite_equals_the_reference(g):
  """A 24 x 32 rendering with three levels and 16 vis rays, two NaN depths."""
  rendering, rays = _suite_inputs(g)
  cmaps = {'turbo': g['lut/turbo'], 'gray': g['lut/gray']}
  out = vis.visualize_suite(rendering, rays, cmaps=cmaps)
  torch.cuda.synchronize()
  assert sorted(out) == [str(k) for k in g['suite/keys']]
  assert {'color', 'acc', 'color_matte', 'depth_mean', 'depth_median', 'depth_triplet', 'coords_mod', 'ray_colors', 'ray_weights',
          'color_corrected', 'normals', 'normals_pred', 'roughness'} == set(out)
  for k in ('color', 'acc', 'color_corrected'):
    assert np.array_equal(_np(out[k]), g[f'suite/out/{k}'])
  assert (_np(out['acc'])[[3, 20], [5, 30]] == 0).all()                           # acc is zeroed where distance_mean is NaN
  for k in ('color_matte', 'normals', 'normals_pred', 'roughness', 'coords_mod'):
    got, want = _np(out[k]), g[f'suite/out/{k}']
    print(f'{k}: max diff {np.nanmax(np.abs(got - want)):.3g}')
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= PIX_BOUND
  for k in ('depth_mean', 'depth_median'):
    _check_lut_image(k, _np(out[k]), g[f'suite/out/{k}'], g['lut/turbo'])
  got = _np(out['depth_triplet'])
  print(f'depth_triplet: max diff {np.abs(got - g["suite/out/depth_triplet"]).max():.3g}')
  assert np.abs(got - g['suite/out/depth_triplet']).max() <= PIX_BOUND
  # the ray panels: 16 rays x (3 levels x 41 rows + a strip) - 1 rows, 2048 columns
  rows, step = g['suite/panel_rows'], int(g['suite/panel_col_step'])
  for k in ('ray_colors', 'ray_weights'):
    full = _np(out[k])
    assert full.shape == (16 * (3 * 41 + 1) - 1, 2048, 3)
    for r in rows[:-1]:
      assert (full[r:r + 41] == full[r]).all()                                    # a (ray, level) block repeats one row
    got, want = full[rows][:, ::step], g[f'suite/out/{k}']
    d = float(np.abs(got - want).max())
    print(f'{k}: largest difference to the float64 record {d:.6g} over {got.size} sampled values (bound {RAY_PANEL_BOUND[k]:.3g}), '
          f'differing by more than 1e-5: {int((np.abs(got - want) > 1e-5).sum())}')
    assert d <= RAY_PANEL_BOUND[k]
  assert (_np(out['ray_colors'])[3 * 41] == float(np.float32(0.8))).all()                            # the strip after a ray's levels: background
  assert (_np(out['ray_weights'])[3 * 41] == [1., 0., 0.]).all()                  # alpha 0: the null colour


# ----------------------------------------------------------------------------- spherical camera, dataset


@pytest.mark.parametrize('tag', ['sph_6x9', 'sph_17x32'])
def test_spherical_rays_kernel_equals_the_reference(g, tag):
  H, W = (int(v) for v in tag[4:].split('x'))
  rays = camera_utils.cast_spherical_rays(_dev(g[f'{tag}/c2w']), H, W, 0.2, 1e6)
  torch.cuda.synchronize()
  for k, c in (('origins', 3), ('directions', 3), ('viewdirs', 3), ('radii', 1), ('imageplane', 2)):
    got, want = _np(getattr(rays, k)), g[f'{tag}/{k}']
    err = np.abs(got - want) / ref.ulp32(want)
    print(f'{tag} {k}: shape {got.shape}, largest error {err.max():.3g} float32 ulp')
    assert got.shape == (H, W, c) and err.max() <= 1.0
  assert not _np(rays.imageplane).any()
  assert np.array_equal(_np(rays.viewdirs), _np(rays.directions))
  assert rays.lossmult.shape == (H, W, 1) and (rays.lossmult == 1).all() and (rays.near == 0.2).all() and (rays.far == 1e6).all()
  assert rays.cam_idx.dtype == torch.int32 and not rays.cam_idx.any()


@pytest.mark.parametrize('camtype', ['pano', 'perspective'])
def test_procedural_render_path_dataset_on_the_device(camtype):
  cfg = configs.load_preset('blender_256', ["Config.dataset_loader = 'procedural'", 'Config.render_path = True',
                                            'Config.render_path_frames = 3', 'Config.render_resolution = (20, 12)',
                                            f"Config.render_camtype = '{camtype}'"])
  ds = datasets.load_dataset('test', None, cfg, device='cuda')
  assert ds.size == 3 and (ds.width, ds.height) == (20, 12)
  for b in (ds.generate_ray_batch(1), next(ds)):
    assert b.rgb is None
    r = b.rays
    assert r.origins.shape == (12, 20, 3) and r.directions.shape == (12, 20, 3) and r.viewdirs.shape == (12, 20, 3)
    assert r.radii.shape == (12, 20, 1) and r.imageplane.shape == (12, 20, 2) and r.near.shape == (12, 20, 1)
    assert torch.isfinite(r.directions).all() and (r.radii > 0).all()
  want = ds.camtoworlds[1, :, 3].cpu()
  assert torch.equal(ds.generate_ray_batch(1).rays.origins.cpu()[5, 7], want)
  if camtype == 'pano':
    d = ds.generate_ray_batch(0).rays.directions
    assert (d.norm(dim=-1) - 1).abs().max() <= 1e-6                               # unit directions all around
    assert (d[0, 0] - d[0, 10]).abs().max() <= 1e-6 and (d[6, 0] + d[6, 10]).abs().max() <= 1e-6     # the pole; half a turn apart


# ----------------------------------------------------------------------------- render.py


def test_render_script_end_to_end(tmp_path, g):
  """render.py on the procedural scene from a checkpoint of the initial state (no training): the reference's files for three
  path frames, the video-frame folders, --vis; a second run skips; a strided job writes its own frames only."""
  from PIL import Image
  ck = str(tmp_path / 'exp' / 'scene')
  binds = ["Config.dataset_loader = 'procedural'", f"Config.checkpoint_dir = '{ck}'", 'NerfMLP.net_width = 128', 'PropMLP.net_width = 128',
           'NerfMLP.bottleneck_width = 128', 'Config.factor = 4', 'Config.render_path = True', 'Config.render_path_frames = 3',
           'Config.render_chunk_size = 4096']
  config = configs.load_preset('blender_256', binds)
  model, state, _, _, _ = train_utils.setup_model(config, 20200823, device='cuda')
  checkpoints.save_checkpoint(ck, model, state, 0)
  lut_file = str(tmp_path / 'luts.npz')
  np.savez(lut_file, turbo=g['lut/turbo'], gray=g['lut/gray'])
  env = dict(os.environ, PYTHONPATH=ROOT)

  def run(extra_binds=(), extra_args=()):
    args = ['--preset', 'blender_256', '--colormaps', lut_file] + list(extra_args)
    for b in binds + list(extra_binds):
      args += ['--gin_bindings', b]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'render.py')] + args, capture_output=True, text=True, env=env, timeout=600,
                       cwd=ROOT)
    print(r.stdout[-2500:], r.stderr[-2500:])
    assert r.returncode == 0
    return r.stdout

  stdout = run(extra_args=['--vis'])
  assert 'Rendering checkpoint at step 0.' in stdout and 'All files found, creating videos (job 0).' in stdout
  out = os.path.join(ck, 'render', 'path_renders_step_0')
  files = set(os.listdir(out))
  want = {f'{k}_{i:03d}.{e}' for i in range(3) for k, e in (('color', 'png'), ('distance_mean', 'tiff'), ('distance_median', 'tiff'),
                                                              ('acc', 'tiff'))}
  assert want <= files, sorted(want - files)
  assert not any(f.startswith('normals') for f in files)          # (blender_256 has no normals; models with normals write normals_NNN.png)
  assert 'vis_depth_mean_000.png' in files and 'vis_ray_weights_002.png' in files
  acc = np.asarray(Image.open(os.path.join(out, 'acc_001.tiff')))
  assert acc.dtype == np.float32 and acc.shape == (24, 24)
  assert np.asarray(Image.open(os.path.join(out, 'color_001.png'))).shape == (24, 24, 3)
  assert np.asarray(Image.open(os.path.join(out, 'vis_depth_mean_000.png'))).shape == (24, 24, 3)
  for k in ('color', 'acc', 'distance_mean', 'distance_median'):
    folder = os.path.join(ck, 'render', f'scene_exp_path_renders_step_0_{k}')
    assert sorted(os.listdir(folder)) == ['000.png', '001.png', '002.png'], k
  # a distance video frame is the host colourisation of the saved TIFF between frame 0's percentiles (render.py:54-93)
  d0 = np.asarray(Image.open(os.path.join(out, 'distance_mean_000.tiff')), np.float64)
  d1 = np.asarray(Image.open(os.path.join(out, 'distance_mean_001.tiff')), np.float64)
  lo, hi = np.log(np.percentile(d0.reshape(-1), [0.5, 99.5]))
  host = ref.host_colourise(d1, lo, hi, g['lut/turbo'].astype(np.float32).astype(np.float64))
  frame = np.asarray(Image.open(os.path.join(ck, 'render', 'scene_exp_path_renders_step_0_distance_mean', '001.png')))
  differing = int((frame != host).any(-1).sum())
  print(f'distance_mean video frame 1: {differing} of {frame.shape[0] * frame.shape[1]} pixels differ from the host colourisation')
  assert frame.shape == (24, 24, 3) and differing <= max(1, int(LUT_SHARE * 24 * 24))
  assert np.array_equal(np.asarray(Image.open(os.path.join(ck, 'render', 'scene_exp_path_renders_step_0_color', '002.png'))),
                        np.asarray(Image.open(os.path.join(out, 'color_002.png'))))
  grey = np.asarray(Image.open(os.path.join(ck, 'render', 'scene_exp_path_renders_step_0_acc', '000.png')))
  assert grey.shape == (24, 24) and np.array_equal(grey, (np.clip(np.asarray(Image.open(os.path.join(out, 'acc_000.tiff')), np.float64), 0, 1) * 255).astype(np.uint8))
  # second run: frames whose own and next colour image exist are skipped
  stdout = run()
  assert 'Image 0/3 already exists, skipping' in stdout and 'Image 1/3 already exists, skipping' in stdout
  assert 'Evaluating image 3/3' in stdout and 'Evaluating image 1/3' not in stdout
  # a strided job in a fresh folder writes frame 1 only, synchronously
  other = str(tmp_path / 'other')
  stdout = run([f"Config.render_dir = '{other}'", 'Config.render_num_jobs = 2', 'Config.render_job_id = 1',
                'Config.render_save_async = False'])
  files = sorted(os.listdir(os.path.join(other, 'path_renders_step_0')))
  assert files == ['acc_001.tiff', 'color_001.png', 'distance_mean_001.tiff', 'distance_median_001.tiff'], files
  assert 'All files found' not in stdout
  assert os.listdir(os.path.join(other, 'scene_exp_path_renders_step_0_color')) == ['001.png']
  assert not os.path.exists(os.path.join(other, 'scene_exp_path_renders_step_0_distance_mean', '001.png'))   # frame 0 sets the limits
