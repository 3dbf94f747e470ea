"""MLP.__call__ on caller-supplied Gaussians (reference models.py:403-409,604-612): the two kernels of csrc/gaussians.hip
(mnr_ipe_from_gaussians, mnr_ipe_from_gaussians_tangent) and `model.nerf_hp(...)` / `model.prop_hp(...)` on top of them.  -m gpu.

  (a) on Gaussians exported by the ray kernels (no contraction) the rows are those kernels' rows, bit for bit;
  (b) the contraction of a GENERAL covariance and the encoding behind it against oracle.coord in float64;
  (c) the tangent rows under the contraction against torch.func.jvp of the float64 oracle;
  (d) a level's MLP called on that level's exported Gaussians returns the composed model's ray_history, bit for bit;
  (e) the call against the reference's MLP (oracle.models.mlp_apply), within twice the oracle's own bf16 cost;
  (f) the same in Model(dense_precision='fp32') against mlp_apply in float64;
  (g) argument errors, and a call between a training forward pass and its backward pass leaves that state alone.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import configs, geopoly, models
from multinerf_amd import ops as _ops
from oracle import coord as ocoord
from oracle import models as omodels
from oracle import render as orender
from tests import helpers


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')


@pytest.fixture(scope='module')
def ops():
  return _ops


def dev(t):
  return t.cuda()


def _basis(name):
  return torch.as_tensor(geopoly.generate_basis(*name), dtype=torch.float32)


def _bits(t):
  return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ----------------------------------------------------------------------------- (a)


@pytest.mark.parametrize('basis_name,maxdeg', [(('octahedron', 1), 16), (('icosahedron', 2), 12)])
def test_rows_equal_the_ray_kernels_bit_for_bit(ops, basis_name, maxdeg):
  """9 rays x 29 samples = 261 Gaussians (two blocks, the last one partial), warp_contract = False: the means and covariances
  mnr_cast_rays_ipe exports, fed back through mnr_ipe_from_gaussians, give its bf16 rows exactly (zero padding included), and
  mnr_ipe_from_gaussians_tangent gives mnr_cast_rays_ipe_tangent's; the unrounded fp32 rows are mnr_cast_rays_ipe_f32's."""
  gen = torch.Generator().manual_seed(31)
  B, n = 9, 29
  o = torch.rand((B, 3), generator=gen) * 2 - 1
  d = torch.nn.functional.normalize(torch.randn((B, 3), generator=gen), dim=-1) * (1.0 + 0.2 * torch.rand((B, 1), generator=gen))
  radii = 3e-4 + 7e-4 * torch.rand((B,), generator=gen)
  tdist = (2.0 + 4.0 * torch.sort(torch.rand((B, n + 1), generator=gen), -1).values).contiguous()
  basis = _basis(basis_name)
  nfeat = 2 * basis.shape[0] * maxdeg
  ld = (nfeat + 63) // 64 * 64
  kw = dict(min_deg=0, max_deg=maxdeg, ld_feat=ld)
  feat, gm, gc = ops.cast_rays_ipe(dev(tdist), dev(o), dev(d), dev(radii), dev(basis), ray_shape='cone', warp_contract=False,
                                   want_gaussians=True, **kw)
  mine = ops.ipe_from_gaussians(gm, gc, dev(basis), warp_contract=False, **kw)
  torch.cuda.synchronize()
  assert mine.shape == (B * n, ld)
  np.testing.assert_allclose(mine.cpu().float().numpy(), feat.cpu().float().numpy(), atol=0, rtol=0)
  assert torch.equal(_bits(mine.cpu()), _bits(feat.cpu()))
  assert (mine.cpu().float()[:, nfeat:] == 0).all()
  assert feat.float().abs().max().item() > 0.5                                     # (not a comparison of zeros)
  tang = ops.cast_rays_ipe_tangent(dev(tdist), dev(o), dev(d), dev(radii), dev(basis), ray_shape='cone', **kw)
  mine_t = ops.ipe_from_gaussians_tangent(gm, gc, dev(basis), warp_contract=False, **kw)
  torch.cuda.synchronize()
  assert mine_t.shape == (3 * B * n, ld)
  np.testing.assert_allclose(mine_t.cpu().float().numpy(), tang.cpu().float().numpy(), atol=0, rtol=0)
  assert torch.equal(_bits(mine_t.cpu()), _bits(tang.cpu()))
  assert (mine_t.cpu().float()[:, nfeat:] == 0).all()
  feat32 = ops.cast_rays_ipe_f32(dev(tdist), dev(o), dev(d), dev(radii), dev(basis), ray_shape='cone', warp_contract=False,
                                 min_deg=0, max_deg=maxdeg)
  _, mine32 = ops.ipe_from_gaussians(gm, gc, dev(basis), warp_contract=False, want_f32=True, **kw)
  torch.cuda.synchronize()
  assert mine32.shape == feat32.shape == (B * n, nfeat) and mine32.dtype == torch.float32
  assert torch.equal(_bits(mine32.cpu()), _bits(feat32.cpu()))
  assert feat32.abs().max().item() > 0.5


# ----------------------------------------------------------------------------- (b), (c)


@functools.lru_cache(maxsize=None)
def _general_gaussians():
  """261 seeded Gaussians: a third of the means inside the unit ball, a third at radius 1.1 - 4, a third log-uniform in
  10 - 1e5, one mean exactly zero; covariances A A^T with A ~ 0.05 radius N(0, 1), one all-zero.  Shared, never written."""
  gen = torch.Generator().manual_seed(20240611)
  M, third = 261, 87
  r = torch.cat([torch.rand(third, generator=gen), 1.1 + 2.9 * torch.rand(third, generator=gen),
                 10.0 ** (1.0 + 4.0 * torch.rand(third, generator=gen))])
  x = torch.nn.functional.normalize(torch.randn((M, 3), generator=gen), dim=-1) * r[:, None]
  x[5] = 0.0
  A = 0.05 * r[:, None, None] * torch.randn((M, 3, 3), generator=gen)
  cov = A @ A.transpose(-1, -2)
  cov[100] = 0.0
  return x.float().contiguous(), cov.float().contiguous()


@pytest.mark.parametrize('basis_name,maxdeg', [(('icosahedron', 2), 12), (('octahedron', 1), 16), (('octahedron', 1), 16),
                                               (('icosahedron', 1), 10), (('icosahedron', 3), 4)])
def test_general_contraction_against_float64(ops, basis_name, maxdeg):
  """coord.track_linearize(coord.contract) for a general symmetric covariance, then lift_and_diagonalize and
  integrated_pos_enc: post-warp Gaussians and fp32 features against oracle.coord in float64 on the same float32 inputs, by the
  rule of tests/test_gpu_kernels.py::test_cast_rays_ipe: the kernel may be at most 4x as far from float64 as the float32 oracle
  is, with floors 2e-6 (means), 1e-5 (covariance, relative to the row's largest entry) and 2e-6 2^l + 1e-6 (features of degree
  l); the bf16 rows are the rounding of the fp32 features.  (The basis / degree pairs are test_cast_rays_ipe's five.)"""
  x, cov = _general_gaussians()
  M = x.shape[0]
  basis = _basis(basis_name)
  K = basis.shape[0]
  nfeat = 2 * K * maxdeg
  ld = (nfeat + 63) // 64 * 64
  feat, f32, gm, gc = ops.ipe_from_gaussians(dev(x), dev(cov), dev(basis), warp_contract=True, min_deg=0, max_deg=maxdeg,
                                             ld_feat=ld, want_f32=True, want_gaussians=True)
  torch.cuda.synchronize()
  feat, f32, gm, gc = feat.cpu(), f32.cpu(), gm.cpu(), gc.cpu()
  assert torch.isfinite(f32).all() and torch.isfinite(gc).all()
  m64, c64 = ocoord.track_linearize(ocoord.contract, x.double(), cov.double())
  m32, c32 = ocoord.track_linearize(ocoord.contract, x, cov)
  em_k, em_o = (gm.double() - m64).abs().max().item(), (m32.double() - m64).abs().max().item()
  print(f'means: kernel {em_k:.2e} fp32-oracle {em_o:.2e}')
  assert em_k <= max(4 * em_o, 2e-6), (em_k, em_o)
  c64r = c64.reshape(M, 9)
  sc = c64r.abs().max(-1, keepdim=True).values.clamp_min(1e-30)
  ec_k = ((gc.double() - c64r).abs() / sc).max().item()
  ec_o = ((c32.double().reshape(M, 9) - c64r).abs() / sc).max().item()
  print(f'cov rel err: kernel {ec_k:.2e} fp32-oracle {ec_o:.2e}')
  assert ec_k <= max(4 * ec_o, 1e-5), (ec_k, ec_o)
  assert (gm[5] == 0).all() and (gc[100] == 0).all()                                # (the zero mean, the zero covariance)
  bT = basis.T.contiguous()
  lmk, lvk = ocoord.lift_and_diagonalize(gm.double(), gc.double().reshape(M, 3, 3), bT.double())
  ref64_k = ocoord.integrated_pos_enc(lmk, lvk, 0, maxdeg)                          # fp64 from the kernel's Gaussians
  lmo, lvo = ocoord.lift_and_diagonalize(m32.double(), c32.double(), bT.double())
  ref64_o = ocoord.integrated_pos_enc(lmo, lvo, 0, maxdeg)                          # fp64 from the oracle's Gaussians
  lm32, lv32 = ocoord.lift_and_diagonalize(m32, c32, bT)
  ref32 = ocoord.integrated_pos_enc(lm32, lv32, 0, maxdeg).double()
  got = f32.double()
  for l in range(maxdeg):
    cols = [h * K * maxdeg + l * K + k for h in (0, 1) for k in range(K)]
    e_kernel = (got[:, cols] - ref64_k[:, cols]).abs().max().item()
    e_oracle = (ref32[:, cols] - ref64_o[:, cols]).abs().max().item()
    assert e_kernel <= max(4 * e_oracle, 2e-6 * 2**l + 1e-6), (l, e_kernel, e_oracle)
  if feat.dtype == torch.bfloat16:
    np.testing.assert_allclose(feat.float()[:, :nfeat].numpy(), f32.to(torch.bfloat16).float().numpy(), atol=0, rtol=0)
  assert (feat.float()[:, nfeat:] == 0).all()


def test_tangent_rows_under_the_general_contraction(ops):
  """d features / d mean_c with the covariance an input held fixed (what jax.value_and_grad(predict_density) differentiates,
  models.py:441-446,473-492) against torch.func.jvp of the float64 oracle, by the rule of tests/test_gpu_refnerf.py::
  test_tangent_features_under_the_contraction: column-relative error below 2e-2, scale floor 1e-3.  Samples with
  | |x| - 1 | < 1e-3 (the contraction's kink) are left out: at most 2 % of them."""
  x, cov = _general_gaussians()
  M, maxdeg = x.shape[0], 12
  basis = _basis(('icosahedron', 2))
  F = 2 * basis.shape[0] * maxdeg
  ld = (F + 127) // 128 * 128
  tang = ops.ipe_from_gaussians_tangent(dev(x), dev(cov), dev(basis), warp_contract=True, min_deg=0, max_deg=maxdeg, ld_feat=ld)
  torch.cuda.synchronize()
  tang = tang.cpu().float()
  assert tang.shape == (3 * M, ld) and (tang[:, F:] == 0).all() and torch.isfinite(tang).all()
  keep = (x.double().norm(dim=-1) - 1).abs() >= 1e-3
  assert (~keep).sum().item() <= 0.02 * M
  bT, c64 = basis.T.contiguous().double(), cov.double()

  def feats(mu):
    mu2, cv2 = ocoord.track_linearize(ocoord.contract, mu, c64)
    lm, lv = ocoord.lift_and_diagonalize(mu2, cv2, bT)
    return ocoord.integrated_pos_enc(lm, lv, 0, maxdeg)

  for cdir in range(3):
    e = torch.zeros((M, 3), dtype=torch.float64)
    e[:, cdir] = 1
    _, ref = torch.func.jvp(feats, (x.double(),), (e,))
    ref = ref[keep]
    got = tang[cdir * M:(cdir + 1) * M, :F].double()[keep]
    scale = ref.abs().max(0, keepdim=True).values.clamp_min(1e-3)
    err = ((got - ref).abs() / scale).max().item()
    print(f'tangent rows of general Gaussians under the contraction, d/d mean_{cdir}: max column-relative error {err:.2e}')
    assert err < 2e-2


# ----------------------------------------------------------------------------- models


KEYS = ('density', 'rgb', 'raw_grad_density', 'grad_pred', 'normals', 'normals_pred', 'roughness')


def _model(name, extra, seed=3, **model_kw):
  """A built model with the oracle's seeded parameters (non-zero biases) bound -> (cfg, model, oracle hparams, params)."""
  cfg = configs.load_preset(name, list(extra))
  model = models.Model(config=cfg, **model_kw).build('cuda')
  om, on, op = helpers.oracle_hparams(model)
  params = omodels.init_params(om, on, op, seed=seed)
  g = torch.Generator().manual_seed(seed + 1)
  for mname, mod in params.items():
    if mname in ('exposure_scaling_offsets', 'Embed_0'):
      continue
    for d in mod.values():
      d['bias'] = 0.05 * torch.randn(d['bias'].shape, generator=g)
  model.bind({'flat': model.flat_from_tree(params)})
  return cfg, model, (om, on, op), params


W128 = ['NerfMLP.net_width = 128', 'PropMLP.net_width = 128']


@pytest.mark.parametrize('name,extra', [('blender_256', []), ('blender_refnerf', []), ('llff_raw', []),
                                        ('llff_raw', ['NerfMLP.disable_density_normals = False'])])
def test_level_mlp_on_exported_gaussians_equals_ray_history(monkeypatch, name, extra):
  """Model.__call__ on 8 rays (rng None), then every level's MLP called on that level's own Gaussians (exported by
  mnr_cast_rays_ipe from the level's tdist; these presets have no contraction): every non-None output equals the level's
  ray_history entry EXACTLY, the feature rows being the same bits (test (a)) and every kernel behind them the level loop's own.

  That includes the one level Model.__call__ does not run on a feature matrix: a density-only proposal MLP on the fused chain
  (blender_256's PropMLP_0) is evaluated by render / eval passes with its featurisation INSIDE the chain kernel
  (mnr_mlp_chain_fwd_ipe), whose layer 0 accumulates over K group-major (include/mnerf.h); the stand-alone call moves its
  feature columns into that order and runs the chain on the same group-major operand (Model._chain_forward_grouped), so the
  MFMA accumulation order is that kernel's.  (The plain feature-matrix chain differs from it by 5.5e-5 = 1835 float32 ulps in the density on
  these inputs, measured on the kernel-source simulator.)  As an extra, with models._FUSED_IPE = False both Model.__call__ and the call take the feature-matrix form
  (the form every training step runs), and must agree exactly there too."""
  cfg, model, _, _ = _model(name, W128 + extra)
  rays = helpers.synthetic_rays(8, near=cfg.near, far=cfg.far).rays.map(lambda t: t.cuda())

  def level_outputs(hist):
    outs = []
    for i, h in enumerate(hist):
      is_prop = i < model.num_levels - 1
      plan, mlp = (model.prop_plan, model.prop_hp) if is_prop else (model.nerf_plan, model.nerf_hp)
      hp = plan.hp
      assert hp.warp_fn is None
      _, gm, gc = _ops.cast_rays_ipe(h['tdist'].contiguous(), rays.origins, rays.directions, rays.radii.reshape(-1).contiguous(),
                                     plan.basis_dev, ray_shape=model.ray_shape, warp_contract=False, min_deg=hp.min_deg_point,
                                     max_deg=hp.max_deg_point, ld_feat=plan.ldF, disable_integration=model.disable_integration,
                                     want_gaussians=True)
      n = h['tdist'].shape[-1] - 1
      outs.append(mlp(None, (gm.view(8, n, 3), gc.view(8, n, 3, 3)), viewdirs=rays.viewdirs if plan.use_viewdirs else None,
                      imageplane=rays.imageplane))
    return outs

  _, hist = model(None, rays, 1.0, False)
  outs = level_outputs(hist)
  torch.cuda.synchronize()
  fused = [i < model.num_levels - 1 and model._ipe_chain_ok(model.prop_plan) for i in range(model.num_levels)]
  assert any(fused) == (name == 'blender_256') and not fused[-1]
  compared = 0
  for i, (h, out) in enumerate(zip(hist, outs)):
    assert set(out) == set(KEYS)
    for k in KEYS:
      assert (out[k] is None) == (h[k] is None), (i, k)
      if out[k] is None:
        continue
      assert out[k].shape == h[k].shape, (i, k)
      assert torch.equal(out[k], h[k]), (name, i, k, (out[k] - h[k]).abs().max().item())
      compared += 1
  assert compared >= 2
  assert hist[-1]['density'].abs().max().item() > 0 and hist[-1]['rgb'].abs().max().item() > 0
  if any(fused):
    monkeypatch.setattr(models, '_FUSED_IPE', False)
    _, hist2 = model(None, rays, 1.0, False)
    outs2 = level_outputs(hist2)
    torch.cuda.synchronize()
    for i, (h, out) in enumerate(zip(hist2, outs2)):
      for k in KEYS:
        if out[k] is not None:
          assert torch.equal(out[k], h[k]), (name, i, k, (out[k] - h[k]).abs().max().item())


# ----------------------------------------------------------------------------- (e), (f)


def _oracle_inputs(cfg, model, plan, B=8, n=32, seed=11):
  """Pre-warp Gaussians of 8 rays x 32 samples from oracle.render.cast_rays in float32, view directions, a GLO vector and
  the two noise tensors (CPU)."""
  g = torch.Generator().manual_seed(seed)
  rays = helpers.synthetic_rays(B, near=cfg.near, far=cfg.far).rays
  s = torch.sort(torch.rand((B, n + 1), generator=g), -1).values
  near, far = float(cfg.near), float(cfg.far)
  if near > 0 and far / near > 100:
    tdist = 1.0 / (s / min(far, 1e3) + (1 - s) / near)                # reciprocal spacing: samples in and far beyond the unit ball
    tdist = torch.sort(tdist, -1).values
  else:
    tdist = near + s * (far - near)
  means, covs = orender.cast_rays(tdist.float(), rays.origins, rays.directions, rays.radii, model.ray_shape, diag=False)
  glo = torch.randn((B, plan.glo), generator=g) * 0.5 if plan.glo > 0 else None
  dn = torch.randn((B, n), generator=g)
  bn = torch.randn((B, n, plan.hp.bottleneck_width), generator=g) if plan.has_rgb and plan.use_viewdirs else None
  return means.float().contiguous(), covs.float().contiguous(), (rays.viewdirs if plan.use_viewdirs else None), glo, dn, bn


def _call_both(model, which, params, inputs, dtypes):
  """The kernel's MLP call and the oracle's mlp_apply for each (float dtype, dense_dtype) of `dtypes`."""
  means, covs, vd, glo, dn, bn = inputs
  plan, mlp = (model.prop_plan, model.prop_hp) if which == 'prop' else (model.nerf_plan, model.nerf_hp)
  om, on, op = helpers.oracle_hparams(model)
  omlp = op if (which == 'prop' and op is not None) else on
  c = lambda t: None if t is None else t.cuda()
  noise = {'density_noise': dn}
  if bn is not None:
    noise['bottleneck_noise'] = bn
  got = mlp(None, (c(means), c(covs)), viewdirs=c(vd), glo_vec=c(glo), noise=noise)
  torch.cuda.synchronize()
  refs = []
  for fdt, ddt in dtypes:
    f = lambda t: None if t is None else t.to(fdt)
    p = params[plan.module_name]
    p = helpers.to_float64(p) if fdt == torch.float64 else p
    r = omodels.mlp_apply(omlp, p, (f(means), f(covs)), viewdirs=f(vd), glo_vec=f(glo), density_noise=f(dn), bottleneck_noise=f(bn),
                          dense_dtype=ddt)
    refs.append({k: (None if v is None else v.detach().double()) for k, v in r.items()})
  return {k: (None if v is None else v.cpu().double()) for k, v in got.items()}, refs


E_360 = ['NerfMLP.net_width = 256', 'PropMLP.net_width = 128', 'Model.num_glo_features = 4', 'NerfMLP.bottleneck_noise = 0.2',
         'NerfMLP.density_noise = 0.5']


@pytest.mark.parametrize('name,extra,which', [('360', E_360, 'prop'), ('360', E_360, 'nerf'), ('blender_refnerf', [], 'nerf'),
                                              ('llff_raw', ['NerfMLP.disable_density_normals = False'], 'nerf')])
def test_call_against_the_reference_mlp(name, extra, which):
  """oracle.models.mlp_apply on the same pre-warp Gaussians, view directions, GLO vector and noise: per output, max norm,
  |kernel - oracle_fp32| <= 2 |oracle_bf16 - oracle_fp32| + 1e-6 scale (scale: the largest fp32-oracle magnitude of that
  output; the factor 2 is the project's "within 2x its own bf16 cost", tests/test_gpu_model.py).  At random initialisation the
  bf16 cost of raw_grad_density and normals is of the order of the values themselves, so for those two this only excludes
  gross errors; the fp32-mode test below is the sharp one."""
  cfg, model, _, params = _model(name, extra)
  plan = model.prop_plan if which == 'prop' else model.nerf_plan
  got, (r32, rbf) = _call_both(model, which, params, _oracle_inputs(cfg, model, plan),
                               [(torch.float32, None), (torch.float32, torch.bfloat16)])
  checked = 0
  for k in KEYS:
    assert (got[k] is None) == (r32[k] is None), k
    if got[k] is None:
      continue
    scale = r32[k].abs().max().item()
    err = (got[k] - r32[k]).abs().max().item()
    cost = (rbf[k] - r32[k]).abs().max().item()
    print(f'MLPCALL {name}/{which} {k}: |kernel - oracle_fp32| {err:.3e}  |oracle_bf16 - oracle_fp32| {cost:.3e}  (scale {scale:.3e})')
    assert err <= 2 * cost + 1e-6 * scale, (k, err, cost, scale)
    checked += 1
  assert checked >= 2 and got['density'].abs().max().item() > 0


F_360 = ['NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'Model.num_glo_features = 4', 'NerfMLP.bottleneck_noise = 0.2',
         'NerfMLP.density_noise = 0.5']
F32_SEED = 11          # (the seed of _oracle_inputs; the share of samples with a small density gradient is asserted below)


@pytest.mark.parametrize('name,extra', [('blender_refnerf', []), ('360', F_360)])
def test_call_in_fp32_mode_against_float64(name, extra):
  """Model(dense_precision='fp32') (the fp32-Dense debug build; csrc/gaussians.hip is part of it) against mlp_apply in float64
  on the same float32 inputs: per output max(2e-4 scale, 2 |oracle_fp32 - oracle_fp64|), helpers.check_fp32_mode_gradient's
  grad_tol and cost_factor.  `normals` (a normalised vector) are compared only where the float64 |raw_grad_density| is at
  least 1e-2 of its maximum; at most 10 % of the samples may fall under that."""
  cfg, model, _, params = _model(name, extra, dense_precision='fp32')
  got, (r64, r32) = _call_both(model, 'nerf', params, _oracle_inputs(cfg, model, model.nerf_plan, seed=F32_SEED),
                               [(torch.float64, None), (torch.float32, None)])
  for k in KEYS:
    assert (got[k] is None) == (r64[k] is None), k
    if got[k] is None:
      continue
    a, r, o = got[k], r64[k], r32[k]
    if k == 'normals':
      gnorm = r64['raw_grad_density'].norm(dim=-1)
      ok = gnorm >= 1e-2 * gnorm.max()
      small = 1.0 - ok.double().mean().item()
      print(f'MLPCALL-F32 {name} normals: {small:.3f} of the samples have |raw_grad_density| < 1e-2 max')
      assert small <= 0.10
      a, r, o = a[ok], r[ok], o[ok]
    scale = r.abs().max().item()
    err = (a - r).abs().max().item()
    cost = (o - r).abs().max().item()
    print(f'MLPCALL-F32 {name} {k}: |kernel_fp32 - oracle_fp64| {err:.3e}  |oracle_fp32 - oracle_fp64| {cost:.3e}  (scale {scale:.3e})')
    assert err <= max(2e-4 * scale, 2 * cost), (k, err, cost, scale)


# ----------------------------------------------------------------------------- (g)


@functools.lru_cache(maxsize=None)
def _small_360():
  return _model('360', ['NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'Model.num_glo_features = 4'])


def _some_gaussians(B=2, n=32):
  g = torch.Generator().manual_seed(5)
  means = torch.randn((B, n, 3), generator=g)
  A = 0.05 * torch.randn((B, n, 3, 3), generator=g)
  return means.cuda(), (A @ A.transpose(-1, -2)).contiguous().cuda(), torch.nn.functional.normalize(torch.randn((B, 3), generator=g), dim=-1).cuda()


def test_argument_errors():
  cfg, model, _, _ = _small_360()
  means, covs, vd = _some_gaussians()
  glo = torch.zeros((2, 4)).cuda()
  with pytest.raises(ValueError, match='covs'):
    model.nerf_hp(None, (means, covs[..., 0]), viewdirs=vd, glo_vec=glo)          # a diagonal [..., n, 3]
  with pytest.raises(ValueError, match='viewdirs'):
    model.nerf_hp(None, (means, covs), glo_vec=glo)
  with pytest.raises(ValueError, match='glo_vec'):
    model.nerf_hp(None, (means, covs), viewdirs=vd)
  with pytest.raises(ValueError, match='float32'):
    model.nerf_hp(None, (means.double(), covs.double()), viewdirs=vd, glo_vec=glo)
  out = model.prop_hp(None, (means, covs))                                        # the proposal MLP reads neither ...
  out2 = model.prop_hp(None, (means, covs), viewdirs=vd, glo_vec=glo)             # ... and ignores both, as the reference does
  assert torch.equal(out['density'], out2['density'])
  assert out['density'].shape == (2, 32) and out['rgb'].shape == (2, 32, 3) and (out['rgb'] == 0).all()
  assert all(out[k] is None for k in KEYS[2:])
  unbuilt = models.Model(config=cfg)
  with pytest.raises(RuntimeError, match='not attached'):
    unbuilt.nerf_hp(None, (means, covs), viewdirs=vd, glo_vec=glo)
  built = models.Model(config=cfg).build('cuda')                                  # built, nothing bound
  with pytest.raises(RuntimeError, match='bound'):
    built.nerf_hp(None, (means, covs), viewdirs=vd, glo_vec=glo)


def test_host_tensors_are_refused():
  _, model, _, _ = _small_360()
  means, covs, vd = _some_gaussians()
  with pytest.raises(ValueError, match='device tensor'):
    model.prop_hp(None, (means.cpu(), covs.cpu()))


def test_seeded_noise_is_reproducible_and_rng_none_is_deterministic():
  cfg, model, _, _ = _model('360', ['NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'NerfMLP.bottleneck_noise = 0.2',
                                    'NerfMLP.density_noise = 0.5'])
  means, covs, vd = _some_gaussians()
  a = model.nerf_hp(None, (means, covs), viewdirs=vd)
  b = model.nerf_hp(None, (means, covs), viewdirs=vd)
  c = model.nerf_hp(7, (means, covs), viewdirs=vd)
  d = model.nerf_hp(7, (means, covs), viewdirs=vd)
  e = model.nerf_hp(torch.Generator(device=model.device).manual_seed(7), (means, covs), viewdirs=vd)
  for k in ('density', 'rgb'):
    assert torch.equal(a[k], b[k]) and torch.equal(c[k], d[k]) and torch.equal(c[k], e[k])
    assert not torch.equal(a[k], c[k])


def test_call_between_forward_and_backward_leaves_the_training_state_alone():
  """After a training forward pass (Model._saved, what train_utils' step keeps for its backward pass), calls of both MLPs leave
  _saved the same objects, every ('lvl', ...) workspace buffer the same values, and _glo_cam / _T_pre what they were."""
  cfg, model, _, _ = _small_360()
  rays = helpers.synthetic_rays(8, near=cfg.near, far=cfg.far).rays.map(lambda t: t.cuda())
  model(torch.Generator(device=model.device).manual_seed(1), rays, 0.5, False, zero_glo=False, keep_for_backward=True)
  saved = model._saved
  ids = [(k, id(v)) for lv in saved['levels'] for k, v in lv.items()] + [(k, id(v)) for k, v in saved.items()]

  def is_lvl(key):
    return isinstance(key[0], tuple) and len(key[0]) > 0 and (key[0][0] == 'lvl' or (isinstance(key[0][0], tuple) and key[0][0][:1] == ('lvl',)))

  lvl = {k: t.clone() for k, t in model._ws.items() if torch.is_tensor(t) and is_lvl(k)}
  assert len(lvl) >= 4
  cam, had_tpre = model._glo_cam, hasattr(model, '_T_pre')
  assert cam is not None
  means, covs, vd = _some_gaussians()
  model.nerf_hp(3, (means, covs), viewdirs=vd, glo_vec=torch.ones((2, 4)).cuda())
  model.prop_hp(None, (means, covs))
  torch.cuda.synchronize()
  assert model._saved is saved
  assert ids == [(k, id(v)) for lv in saved['levels'] for k, v in lv.items()] + [(k, id(v)) for k, v in saved.items()]
  assert model._glo_cam is cam and hasattr(model, '_T_pre') == had_tpre
  for k, t in lvl.items():
    assert torch.equal(model._ws[k], t), k
  assert not any(is_lvl(k) for k in model._ws if k not in lvl and not (isinstance(k, tuple) and k[0] == 'const'))


def test_query_density():
  """Model.query_density(xyz) is the NeRF level's density on points_to_gaussians(xyz, 0.): literally so for a model without
  view directions, and with any view direction / GLO vector for one that reads them (density depends on neither)."""
  g = torch.Generator().manual_seed(9)
  xyz = (torch.randn((300, 3), generator=g) * 2).cuda()
  cfg, model, _, _ = _model('blender_256', W128 + ['Model.use_viewdirs = False'])
  q = model.query_density(xyz)
  ref = model.nerf_hp(None, models.points_to_gaussians(xyz, 0.))['density']
  assert q.shape == (300,) and torch.equal(q, ref) and (q >= 0).all() and q.max().item() > 0
  means, covs = models.points_to_gaussians(xyz, 0.5)
  assert means.shape == (300, 3) and covs.shape == (300, 3, 3)
  assert torch.equal(covs.cpu(), (0.25 * torch.eye(3)).expand(300, 3, 3))
  _, model, _, _ = _small_360()
  q = model.query_density(xyz, std=0.1)
  vd = torch.nn.functional.normalize(torch.randn((3,), generator=g), dim=-1).cuda()
  ref = model.nerf_hp(None, models.points_to_gaussians(xyz, 0.1), viewdirs=vd, glo_vec=torch.ones(4).cuda())['density']
  assert torch.equal(q, ref)
