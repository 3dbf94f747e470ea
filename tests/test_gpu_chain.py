"""The fused per-level Dense chain (csrc/fused_mlp.hip) against the per-layer GEMM path it replaces.  -m gpu.

Both paths feed the same bf16 operands to the same MFMA instruction in the same k order and apply the same bias / ReLU /
rounding, so the layer activations, their 1-bit masks and the dX chain must agree BIT FOR BIT; the Dense(1) head sums
256 products in a different order (fp32) and the weight gradients go through fp32 atomics: those are held to 1e-5.
The composed tests (tests/test_gpu_model.py) hold the fused path to the oracle.
"""

import ctypes as C
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multinerf_amd import configs, models, train_utils
from oracle import models as omodels
from tests import helpers


@pytest.fixture(scope='module', autouse=True)
def _gpu():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')


def _run(use_chain, cfg, flat, batch, noise, monkeypatch):
  monkeypatch.setattr(models, '_USE_CHAIN', use_chain)
  model = models.Model(config=cfg).build('cuda')
  state, _ = train_utils.create_optimizer(cfg, {'flat': flat.clone().cuda(), 'params': None})
  step = train_utils.create_train_step(model, cfg)
  _, stats, _ = step(0, state, batch.map(lambda t: t.cuda()), None, 0.4, 0.0,
                     noise={k: {lv: t.cuda() for lv, t in d.items()} for k, d in noise.items()}, return_grads=True)
  torch.cuda.synchronize()
  saved = model._saved['levels']
  out = dict(grads=stats['_grads'].cpu(), loss=stats.materialize()['loss'], model=model)
  for li, lv in enumerate(saved[:-1]):
    assert bool(lv['mlp'].get('chain')) == use_chain
    out[li] = dict(acts=[a.cpu().clone() for a in lv['mlp']['acts']], bits=[b.cpu().clone() for b in lv['mlp']['bits']],
                   raw=lv['mlp']['raw_density'].cpu().clone(), sdist=lv['sdist'].cpu().clone(), weights=lv['weights'].cpu().clone())
  return out


@pytest.mark.parametrize('W,bindings,B', [
    (256, ['NerfMLP.net_width = 128'], 24),                                            # 360.gin's PropMLP as is: K0 = 512
    (128, ['NerfMLP.net_width = 128', 'PropMLP.net_width = 128', 'PropMLP.net_depth = 3'], 16),
    (256, ['NerfMLP.net_width = 128', 'PropMLP.basis_shape = "octahedron"', 'PropMLP.basis_subdivisions = 1',
           'PropMLP.max_deg_point = 16', 'PropMLP.net_depth = 2'], 8),                 # K0 = 128, two layers
])
def test_fused_chain_equals_per_layer_path(W, bindings, B, monkeypatch):
  cfg = configs.load_preset('360', bindings)
  m0 = models.Model(config=cfg).build('cuda')
  assert m0.prop_plan.W == W and m0._chain_ok(m0.prop_plan)
  om, on, op = helpers.oracle_hparams(m0)
  params = omodels.init_params(om, on, op, seed=5)
  g = torch.Generator().manual_seed(6)
  for mod in params.values():
    for d in mod.values():
      if isinstance(d, dict) and 'bias' in d:
        d['bias'] = 0.05 * torch.randn(d['bias'].shape, generator=g)
  flat = m0.flat_from_tree(params)
  batch = helpers.synthetic_rays(B, near=cfg.near, far=cfg.far)
  noise = helpers.make_noise(m0, B)
  a = _run(True, cfg, flat, batch, noise, monkeypatch)
  b = _run(False, cfg, flat, batch, noise, monkeypatch)
  # level 0 sees identical inputs on both paths: bitwise activations and masks, head to fp32 rounding
  for i, (x, y) in enumerate(zip(a[0]['acts'], b[0]['acts'])):
    assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f'level 0 activation {i}'
  for i, (x, y) in enumerate(zip(a[0]['bits'], b[0]['bits'])):
    assert torch.equal(x, y), f'level 0 mask bits {i}'
  scale = b[0]['raw'].abs().max().item()
  err = (a[0]['raw'] - b[0]['raw']).abs().max().item()
  print(f'W={W}: head |fused - per-layer| = {err:.2e} (|raw| <= {scale:.2e})')
  assert err <= 2e-6 * max(scale, 1.0)
  # the dX chain on identical inputs (level 0's saved masks, a seeded head gradient): bitwise against
  # small_head_bwd + one masked NT GEMM per layer
  model = a['model']
  plan = model.prop_plan
  lv = model._saved['levels'][0]
  M, D = lv['M'], len(plan.trunk)
  bits = lv['mlp']['bits']
  acts = lv['mlp']['acts']
  g_head = (torch.randn((M,), generator=torch.Generator().manual_seed(7)) * 0.01).cuda()
  w_head = flat.cuda()[plan.density.kernel_off:plan.density.kernel_off + W].contiguous()
  dYs = [torch.empty((M, W), dtype=torch.bfloat16, device='cuda') for _ in range(D)]
  Bws = [None] + [model._w(plan, plan.packed[('trunk', i)]['b_off'], models._rup(W, 128), plan.packed[('trunk', i)]['b_ld'])
                  for i in range(1, D)]
  ops = models.ops
  ops.mlp_chain_bwd(g_head, w_head, bits, Bws, dYs, M=M, W=W)
  ref = torch.empty((M, W), dtype=torch.bfloat16, device='cuda')
  ops.small_head_bwd(acts[-1], W, g_head.view(M, 1), w_head.view(W, 1), M=M, K=W, Cn=1, dX=ref, lddx=W, relu_mask=True)
  torch.cuda.synchronize()
  assert torch.equal(ref.view(torch.int16), dYs[-1].view(torch.int16)), 'dY of the last layer'
  for i in reversed(range(1, D)):
    nxt = torch.empty((M, W), dtype=torch.bfloat16, device='cuda')
    ops.gemm_nt(ref, Bws[i], M=M, N=models._rup(W, 128), K1=plan.packed[('trunk', i)]['b_ld'], Cb=nxt, ldcb=W, nb=W,
                bits_in=bits[i - 1])
    torch.cuda.synchronize()
    assert torch.equal(nxt.view(torch.int16), dYs[i - 1].view(torch.int16)), f'dY of layer {i - 1}'
    ref = nxt
  # end to end: downstream of the head's last-ulp differences everything stays close
  np.testing.assert_allclose(a[1]['sdist'].numpy(), b[1]['sdist'].numpy(), atol=2e-5)
  assert abs(a['loss'] - b['loss']) <= 1e-3 * abs(b['loss'])
  for name, lo, hi in model.modules:
    x, y = a['grads'][lo:hi].double(), b['grads'][lo:hi].double()
    rel = ((x - y).norm() / (y.norm() + 1e-30)).item()
    print(f'W={W} {name}: |g(fused) - g(per-layer)| / |g| = {rel:.2e}')
    # (samples move with the head's last ulp: not bitwise.  The proposal MLP's own gradient stays within 1e-3; what is
    # downstream of the moved samples sees bf16 roundings flip, 3-7 % at these 8-24 ray batches)
    assert rel < (2e-2 if name == 'PropMLP_0' else 0.2), (name, rel)


@pytest.mark.parametrize('preset,bindings,B', [
    ('llff_raw', [], 8),                                   # 96 -> 256 x 8, skip concat into layer 5 (K = 256 + 128), heads + view MLP
    ('blender_256', [], 8),                                # the same trunk behind a fused proposal level
    ('llff_raw', ['NerfMLP.net_width = 128', 'NerfMLP.net_depth = 4', 'NerfMLP.skip_layer = 2'], 8),   # W = 128, skip into layer 3
])
def test_fused_trunk_with_skip_equals_per_layer_path(preset, bindings, B, monkeypatch):
  """The 256-wide NeRF trunks (models.py:441-465 incl. the skip concat of :458-459) on the fused chain: activations and
  masks of every layer bit for bit against the per-layer GEMMs on identical inputs, the dX chain from a given dY_last
  bit for bit against one masked NT GEMM per layer, and the whole train step close to the per-layer path."""
  cfg = configs.load_preset(preset, bindings)
  m0 = models.Model(config=cfg).build('cuda')
  plan = m0.nerf_plan
  skips = [i for i, (_, c) in enumerate(plan.trunk) if c]
  if len(skips) != 1:
    pytest.skip(f'{len(skips)} skip layers')
  assert m0._chain_ok(plan) and plan.has_rgb
  om, on, op = helpers.oracle_hparams(m0)
  params = omodels.init_params(om, on, op, seed=5)
  g = torch.Generator().manual_seed(6)
  for mname, mod in params.items():
    if mname in ('exposure_scaling_offsets', 'Embed_0'):
      continue
    for d in mod.values():
      d['bias'] = 0.05 * torch.randn(d['bias'].shape, generator=g)
  flat = m0.flat_from_tree(params)
  batch = helpers.synthetic_rays(B, near=cfg.near, far=cfg.far)
  if cfg.rawnerf_mode:
    batch.rays.exposure_idx = torch.randint(0, 5, (B, 1), generator=g).to(torch.int32)
    batch.rays.exposure_values = 0.5 + torch.rand((B, 1), generator=g)
    batch.rays.lossmult = (torch.rand((B, 3), generator=g) > 0.4).float()
  noise = helpers.make_noise(m0, B)

  def run(use_chain):
    monkeypatch.setattr(models, '_USE_CHAIN', use_chain)
    model = models.Model(config=cfg).build('cuda')
    state, _ = train_utils.create_optimizer(cfg, {'flat': flat.clone().cuda(), 'params': None})
    step = train_utils.create_train_step(model, cfg)
    _, stats, _ = step(0, state, batch.map(lambda t: t.cuda()), None, 0.4, 0.0,
                       noise={k: {lv: t.cuda() for lv, t in d.items()} for k, d in noise.items()}, return_grads=True)
    torch.cuda.synchronize()
    lvs = model._saved['levels']
    lv = [l for l in lvs if l['plan'] is model.nerf_plan][0]          # first level that runs the NeRF MLP
    assert bool(lv['mlp'].get('chain_trunk')) == use_chain
    return dict(grads=stats['_grads'].cpu(), loss=stats.materialize()['loss'], model=model, lv=lv, first=lvs.index(lv),
                acts=[a.cpu().clone() for a in lv['mlp']['acts']], bits=[b.cpu().clone() for b in lv['mlp']['bits']])

  a, b = run(True), run(False)
  if a['first'] == 0:
    # level 0 sees identical inputs on both paths: every layer bit for bit (incl. the skip layer and what follows it)
    for i, (x, y) in enumerate(zip(a['acts'], b['acts'])):
      assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f'activation {i}'
    for i, (x, y) in enumerate(zip(a['bits'], b['bits'])):
      assert torch.equal(x, y), f'mask bits {i}'
  # the dX chain from a seeded dY_last on the chain run's own masks: bitwise against one masked NT GEMM per layer
  model, lv = a['model'], a['lv']
  W, M, D = plan.W, lv['M'], len(plan.trunk)
  bits = lv['mlp']['bits']
  ops = models.ops
  gl = torch.Generator().manual_seed(7)
  keep = ((bits[-1].cpu().int()[..., None] >> torch.arange(8)) & 1).reshape(M, W).bool()
  dy_last = (torch.randn((M, W), generator=gl) * 0.01 * keep).to(torch.bfloat16).cuda()
  dYs = [torch.empty((M, W), dtype=torch.bfloat16, device='cuda') for _ in range(D - 1)] + [None]
  Bws = [None] + [model._w(model.nerf_plan, model.nerf_plan.packed[('trunk', i)]['b_off'], models._rup(W, 128),
                           model.nerf_plan.packed[('trunk', i)]['b_ld']) for i in range(1, D)]
  ops.mlp_chain_bwd(None, None, bits, Bws, dYs, M=M, W=W, dY_in=dy_last)
  ref = dy_last
  for i in reversed(range(1, D)):
    nxt = torch.empty((M, W), dtype=torch.bfloat16, device='cuda')
    ops.gemm_nt(ref, Bws[i], M=M, N=models._rup(W, 128), K1=model.nerf_plan.packed[('trunk', i)]['b_ld'], Cb=nxt, ldcb=W, nb=W,
                bits_in=bits[i - 1])
    torch.cuda.synchronize()
    assert torch.equal(nxt.view(torch.int16), dYs[i - 1].view(torch.int16)), f'dY of layer {i - 1}'
    ref = nxt
  # end to end
  assert abs(a['loss'] - b['loss']) <= 1e-3 * abs(b['loss'])
  for name, lo, hi in model.modules:
    x, y = a['grads'][lo:hi].double(), b['grads'][lo:hi].double()
    rel = ((x - y).norm() / (y.norm() + 1e-30)).item()
    print(f'{preset} {name}: |g(fused trunk) - g(per-layer)| / |g| = {rel:.2e}')
    assert rel < (1e-4 if a['first'] == 0 and cfg.interlevel_loss_mult == 0 and model.single_mlp else 0.2), (name, rel)


@pytest.mark.parametrize('bindings,B,n', [
    ([], 12, 64),                                                                      # 360.gin's PropMLP: K = 21, L = 12, W = 256, contract
    (['PropMLP.net_width = 128', 'PropMLP.net_depth = 2', 'PropMLP.warp_fn = None', 'PropMLP.basis_shape = "octahedron"',
      'PropMLP.basis_subdivisions = 1', 'PropMLP.max_deg_point = 16', 'Model.ray_shape = "cylinder"'], 8, 32),   # K = 9? / L = 16, W = 128, no warp
])
def test_chain_with_in_kernel_ipe_equals_feature_matrix_path(bindings, B, n):
  """mnr_mlp_chain_fwd_ipe (layer 0's IPE features built in LDS, four degrees at a time; render.py:103-127 + coord.py:102-133
  fused with models.py:441-465) against mnr_cast_rays_ipe + mnr_mlp_chain_fwd.  The features are the same bf16 values; only
  layer 0's fp32 accumulation order differs (group-major K), so its bf16 output differs by at most one ulp on a small fraction
  of the elements, and the head stays within 5e-3 of its scale (mean error < 1e-4)."""
  cfg = configs.load_preset('360', ['NerfMLP.net_width = 128'] + bindings)
  model = models.Model(config=cfg).build('cuda')
  plan = model.prop_plan
  assert model._ipe_chain_ok(plan)
  hp, W, D = plan.hp, plan.W, len(plan.trunk)
  flat = model.init_flat_params(seed=3)
  g = torch.Generator().manual_seed(4)
  for d in plan.dense:
    flat[d.bias_off:d.bias_off + d.fan_out] = (0.05 * torch.randn((d.fan_out,), generator=g)).cuda()
  model.pack_weights(flat, ipe=True)
  ops = models.ops
  M = B * n
  origins = (torch.randn((B, 3), generator=g) * 0.3).cuda()
  directions = torch.nn.functional.normalize(torch.randn((B, 3), generator=g), dim=-1).cuda() * 1.3
  radii = (0.002 + 0.002 * torch.rand((B,), generator=g)).cuda()
  tdist = torch.cumsum(0.02 + torch.rand((B, n + 1), generator=g) * 0.3, dim=-1).cuda().contiguous()     # in and beyond the unit ball
  kw = dict(ray_shape=model.ray_shape, warp_contract=(hp.warp_fn == 'contract'), min_deg=hp.min_deg_point, max_deg=hp.max_deg_point)
  feat = ops.cast_rays_ipe(tdist, origins, directions, radii, plan.basis_dev, ld_feat=plan.ldF, **kw)
  bias = lambda d: flat[d.bias_off:d.bias_off + d.fan_out]
  lay = lambda key: model._w(plan, plan.packed[key]['f_off'], plan.packed[key]['n_pad'], plan.packed[key]['f_ld'])
  ref_layers = [(lay(('trunk', i)), bias(d)) for i, (d, _) in enumerate(plan.trunk)]
  ipe_layers = [(lay('trunk0_ipe'), bias(plan.trunk[0][0]))] + ref_layers[1:]
  w_head = lay('density')[0]
  b_head = flat[plan.density.bias_off:plan.density.bias_off + 1]
  # layer 0 alone
  x_ref = torch.empty((M, W), dtype=torch.bfloat16, device='cuda')
  x_ipe = torch.empty((M, W), dtype=torch.bfloat16, device='cuda')
  ops.mlp_chain_fwd(feat, plan.ldF, ref_layers[:1], M=M, W=W, acts=[x_ref])
  ops.mlp_chain_fwd_ipe(tdist, origins, directions, radii, plan.basis_dev, ipe_layers[:1], M=M, W=W, act_last=x_ipe, **kw)
  torch.cuda.synchronize()
  a, b = x_ref.cpu().float(), x_ipe.cpu().float()
  frac = (a != b).float().mean().item()
  # one bf16 ulp of the larger value, or (cancellation: a pre-activation near zero) 1e-5 of the layer's scale
  excess = ((a - b).abs() - torch.maximum(torch.maximum(a.abs(), b.abs()) * 2.0 ** -7, torch.full_like(a, 1e-5 * a.abs().max().item()))).max().item()
  print(f'layer 0: {frac:.2e} of the bf16 outputs differ; max |diff| {(a - b).abs().max().item():.2e} (|x| <= {a.abs().max().item():.2e})')
  assert excess <= 0 and frac < 5e-3
  assert x_ref.float().abs().max().item() > 0.1                                      # (not a comparison of zeros)
  # the whole chain with its density head
  h_ref = torch.empty((M,), dtype=torch.float32, device='cuda')
  h_ipe = torch.empty((M,), dtype=torch.float32, device='cuda')
  ops.mlp_chain_fwd(feat, plan.ldF, ref_layers, M=M, W=W, w_head=w_head, b_head=b_head, head_out=h_ref)
  ops.mlp_chain_fwd_ipe(tdist, origins, directions, radii, plan.basis_dev, ipe_layers, M=M, W=W, w_head=w_head, b_head=b_head,
                        head_out=h_ipe, **kw)
  torch.cuda.synchronize()
  scale = h_ref.abs().max().item()
  err = (h_ref - h_ipe).abs()
  print(f'head: max |fused - matrix| = {err.max().item():.2e}, mean {err.mean().item():.2e} (|raw| <= {scale:.2e})')
  assert err.max().item() <= 5e-3 * scale and err.mean().item() <= 1e-4 * scale


def test_render_with_in_kernel_ipe_equals_feature_matrix_path(monkeypatch):
  """Model.__call__ without a backward pass (render / eval): the proposal levels on mnr_mlp_chain_fwd_ipe against the same
  forward pass with the feature matrices (MNR_FUSED_IPE=0); the composed oracle parity of this path is
  tests/test_gpu_model.py::test_forward_parity, which runs it by default."""
  cfg = configs.load_preset('360', ['NerfMLP.net_width = 128'])
  B = 24
  batch = helpers.synthetic_rays(B, near=cfg.near, far=cfg.far)
  out = {}
  for on in (True, False):
    monkeypatch.setattr(models, '_FUSED_IPE', on)
    model = models.Model(config=cfg).build('cuda')
    flat = model.init_flat_params(seed=3)
    calls = []
    real = models.ops.mlp_chain_fwd_ipe
    monkeypatch.setattr(models.ops, 'mlp_chain_fwd_ipe', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    renderings, hist = model.apply({'flat': flat}, None, batch.rays.map(lambda t: t.cuda()), 0.5, True)
    torch.cuda.synchronize()
    monkeypatch.setattr(models.ops, 'mlp_chain_fwd_ipe', real)
    assert len(calls) == (2 if on else 0)
    out[on] = (renderings[-1]['rgb'].cpu(), [h['sdist'].cpu() for h in hist], renderings[-1]['distance_median'].cpu())
  rgb_a, sd_a, dm_a = out[True]
  rgb_b, sd_b, dm_b = out[False]
  print(f'rgb |fused - matrix| = {(rgb_a - rgb_b).abs().max().item():.2e}, sdist {max((x - y).abs().max().item() for x, y in zip(sd_a, sd_b)):.2e}')
  # (the densities differ in their last bf16-induced digits, the resampled positions move with them)
  for x, y in zip(sd_a, sd_b):
    np.testing.assert_allclose(x.numpy(), y.numpy(), atol=1e-3)
  np.testing.assert_allclose(rgb_a.numpy(), rgb_b.numpy(), atol=5e-3)
  np.testing.assert_allclose(dm_a.numpy(), dm_b.numpy(), rtol=2e-2, atol=1e-3)


@pytest.mark.parametrize('W,K0,depth,tiles,skip', [(128, 128, 2, 20, 0), (256, 64, 3, 12, 0), (128, 64, 3, 10, 2)])
def test_chain_small_grids_change_no_bit(W, K0, depth, tiles, skip):
  """The chain kernels' persistent loop at sizes the simulator finishes: with at most n workgroups (mnr_mlp_chain_set_max_wgs,
  include/mnerf_debug.h) every workgroup walks several tiles, and that must not change one bit of the forward pass (activations,
  masks, head) or of the dX chain.  skip > 0: that layer reads [x | features] (models.py:458-459), the feature segment streamed
  a second time per tile."""
  ops = models.ops
  dbg = ops.L.debug()
  M = tiles * 256
  g = torch.Generator().manual_seed(11)
  bf = torch.bfloat16
  feat = (torch.rand((M, K0), generator=g) * 2 - 1).to(bf).cuda()
  fan_in = lambda i: K0 if i == 0 else (W + K0 if i == skip else W)
  layers = [(((torch.rand((W, fan_in(i)), generator=g) * 2 - 1) * (6.0 / fan_in(i)) ** 0.5).to(bf).cuda(),
             (0.05 * torch.randn((W,), generator=g)).cuda()) for i in range(depth)]
  wh = ((torch.rand((W,), generator=g) * 2 - 1) * 0.15).to(bf).cuda()
  bh = torch.full((1,), 0.01).cuda()
  gh = (torch.randn((M,), generator=g) * 0.01).cuda()
  Bw = [None] + [layers[i][0][:, :W].t().contiguous() for i in range(1, depth)]     # (the dX chain runs over the x segment)

  def run():
    out = torch.empty((M,), device='cuda')
    acts = [torch.empty((M, W), dtype=bf, device='cuda') for _ in range(depth)]
    bits = [torch.empty((M, W // 8), dtype=torch.uint8, device='cuda') for _ in range(depth)]
    dY = [torch.empty((M, W), dtype=bf, device='cuda') for _ in range(depth)]
    ops.mlp_chain_fwd(feat, K0, layers, M=M, W=W, w_head=wh, b_head=bh, head_out=out, acts=acts, bits=bits, skip_layer=skip)
    ops.mlp_chain_bwd(gh, wh.float(), bits, Bw, dY, M=M, W=W)
    torch.cuda.synchronize()
    return [out.cpu()] + [a.cpu().view(torch.int16) for a in acts] + [b.cpu() for b in bits] + [d.cpu().view(torch.int16) for d in dY]

  ref = run()
  assert ref[1].float().abs().max().item() > 0                                      # (not a comparison of zeros)
  try:
    for max_wgs in (24, 5, 1):
      ops.L.check(dbg.mnr_mlp_chain_set_max_wgs(max_wgs))
      got = run()
      for i, (x, y) in enumerate(zip(ref, got)):
        assert torch.equal(x, y), f'max_wgs {max_wgs}: output {i} differs'
  finally:
    ops.L.check(dbg.mnr_mlp_chain_set_max_wgs(0))


# ----------------------------------------------------------------------------- leaf tests: the three chain kernels against fp64
# Called directly (no Model) on seeded tensors, every layer compared with plain fp64 torch on the kernel's OWN previous bf16
# output, so that errors do not compound.  For a Dense layer with fan-in K, z the fp64 pre-activation and
# mag = sum |a| |w| + |b|:
#
#     |got - relu(z)| <= 1/2 ulp_bf16(z) + (K + 1) 2^-23 mag
#
# the one rounding to bf16, plus a worst-case fp32 accumulation in any order at one fp32 ulp per addition (the rounding inside
# an MFMA's 16-product sum is not documented as round-to-nearest).  The fp32 head: (W + 1) 2^-23 (sum |x| |w| + |b|).  The dX
# layers: the layer formula with K = W and no bias.  Where the arithmetic is fully determined the comparison is bit for bit.

_bf = torch.bfloat16
_NAN = float('nan')
_SENT = -7.0                                    # in every output buffer before the launch (a ReLU never writes it)
_SENT_BITS = 0xA5


def _i16(t):
  return t.view(torch.int16)


def _unpack_mask(bits, W):
  """[M, W / 8] uint8 -> [M, W] bool: column n is bit n & 7 of byte n // 8 (include/mnerf.h)."""
  return ((bits.cpu().int()[..., None] >> torch.arange(8)) & 1).reshape(bits.shape[0], W).bool()


def _leaf_bound(z, mag, K):
  _, ex = torch.frexp(z)                                       # |z| = m 2^ex, m in [0.5, 1): ulp_bf16(z) = 2^(ex - 8)
  half_ulp = torch.where(z != 0, torch.ldexp(torch.ones_like(z), ex - 9), torch.zeros_like(z))
  return half_ulp + (K + 1) * 2.0 ** -23 * mag


def _leaf_ratio(got, ref, bound):
  """max |got - ref| / bound in fp64 (NaN when anything is NaN, which then fails `<= 1`)."""
  err = (got.double() - ref).abs()
  return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


class _chain_switches:
  """mnr_mlp_chain_set_deferred / mnr_mlp_chain_set_max_wgs (include/mnerf_debug.h), restored on the way out."""

  def __enter__(self):
    self.dbg = models.ops.L.debug()
    return self

  def set(self, defer=1, max_wgs=0):
    models.ops.L.check(self.dbg.mnr_mlp_chain_set_deferred(defer))
    models.ops.L.check(self.dbg.mnr_mlp_chain_set_max_wgs(max_wgs))

  def __exit__(self, *exc):
    self.set()
    return False


def _leaf_fwd_inputs(W, K0, ld_feat, pad, depth, skip, M, seed=31):
  """Host tensors of one forward case.  Every padding element (columns >= K0 of feat, >= fan_in of a Bt) is NaN."""
  g = torch.Generator().manual_seed(seed)
  feat = torch.full((M, ld_feat), _NAN, dtype=_bf)
  feat[:, :K0] = (torch.rand((M, K0), generator=g) * 2 - 1).to(_bf)
  fan = [K0 if i == 0 else (W + K0 if (skip > 0 and i == skip) else W) for i in range(depth)]
  Bt, bias = [], []
  for i in range(depth):
    w = torch.full((W, fan[i] + pad), _NAN, dtype=_bf)
    w[:, :fan[i]] = ((torch.rand((W, fan[i]), generator=g) * 2 - 1) * (6.0 / fan[i]) ** 0.5).to(_bf)
    Bt.append(w)
    bias.append(0.05 * torch.randn((W,), generator=g))
  wh = ((torch.rand((W,), generator=g) * 2 - 1) * 0.15).to(_bf)
  bh = torch.full((1,), 0.0625 + 0.01)
  return dict(W=W, K0=K0, depth=depth, skip=skip, M=M, fan=fan, feat=feat, Bt=Bt, bias=bias, wh=wh, bh=bh)


def _leaf_fwd_run(inp, want_acts, want_bits, want_head):
  """One mlp_chain_fwd launch.  want_acts / want_bits: one flag per layer.  Every output buffer has a guard row (element)
  behind the M the kernel is given and starts as a sentinel; the guard must survive.  -> host copies (None: not requested)."""
  ops = models.ops
  M, W, depth = inp['M'], inp['W'], inp['depth']
  acts = [torch.full((M + 1, W), _SENT, dtype=_bf, device='cuda') if w else None for w in want_acts]
  bits = [torch.full((M + 1, W // 8), _SENT_BITS, dtype=torch.uint8, device='cuda') if w else None for w in want_bits]
  head = torch.full((M + 1,), _SENT, device='cuda') if want_head else None
  cut = lambda t: None if t is None else t[:M]
  hk = dict(w_head=inp['wh'].cuda(), b_head=inp['bh'].cuda(), head_out=cut(head)) if want_head else {}
  ops.mlp_chain_fwd(inp['feat'].cuda(), inp['K0'], [(w.cuda(), b.cuda()) for w, b in zip(inp['Bt'], inp['bias'])], M=M, W=W,
                    acts=[cut(a) for a in acts], bits=[cut(b) for b in bits], skip_layer=inp['skip'], **hk)
  torch.cuda.synchronize()
  for a in acts:
    assert a is None or bool((a[M] == _SENT).all()), 'activation guard row'
  for b in bits:
    assert b is None or bool((b[M] == _SENT_BITS).all()), 'mask guard row'
  assert head is None or head[M].item() == _SENT, 'head guard element'
  host = lambda t: None if t is None else t[:M].cpu().clone()
  return dict(acts=[host(a) for a in acts], bits=[host(b) for b in bits], head=host(head))


def _leaf_same(ref, got, what):
  """Every output `got` has is `ref`'s, bit for bit."""
  for i, (x, y) in enumerate(zip(ref['acts'], got['acts'])):
    assert y is None or torch.equal(_i16(x), _i16(y)), f'{what}: activation {i}'
  for i, (x, y) in enumerate(zip(ref['bits'], got['bits'])):
    assert y is None or torch.equal(x, y), f'{what}: mask bits {i}'
  assert got['head'] is None or torch.equal(ref['head'].view(torch.int32), got['head'].view(torch.int32)), f'{what}: head'


def _leaf_fwd_check(inp, out, rows=None):
  """Every layer, its masks and the head of a full run against fp64 -> worst error / bound per output."""
  W, K0, depth = inp['W'], inp['K0'], inp['depth']
  sel = slice(None) if rows is None else rows
  f = inp['feat'][:, :K0].double()[sel]
  ratios = []
  for i in range(depth):
    a = f if i == 0 else out['acts'][i - 1].double()[sel]
    if inp['skip'] > 0 and i == inp['skip']:
      a = torch.cat([a, f], dim=1)                                   # [x | features] (models.py:458-459)
    w, b = inp['Bt'][i][:, :inp['fan'][i]].double(), inp['bias'][i].double()
    z = a @ w.T + b
    mag = a.abs() @ w.abs().T + b.abs()
    got = out['acts'][i][sel]
    ratios.append(_leaf_ratio(got, z.clamp(min=0), _leaf_bound(z, mag, inp['fan'][i])))
    assert torch.equal(_unpack_mask(out['bits'][i], W)[sel], got > 0), f'mask bits of layer {i} are not (activation > 0)'
    assert not bool((_i16(got) == -32768).any()), f'layer {i} stores a negative zero'
  x, wh, bh = out['acts'][-1].double()[sel], inp['wh'].double(), inp['bh'].double()
  ratios.append(_leaf_ratio(out['head'][sel], x @ wh + bh, (W + 1) * 2.0 ** -23 * (x.abs() @ wh.abs() + bh.abs())))
  return ratios


def _leaf_fwd_variants(depth):
  """The output combinations fm_copy_out_dispatch (last layer, and every layer with the copy-out in front of the pass) and
  fm_layer_mfma_defer (the copy-out inside the next pass) distinguish: (acts per layer, bits per layer, head)."""
  yes, no = [True] * depth, [False] * depth
  last = [i == depth - 1 for i in range(depth)]
  v = {'acts only': (yes, no, False), 'bits only': (no, yes, False), 'head only': (no, no, True),
       'acts of the last layer, no head': (last, no, False), 'acts + head': (yes, no, True), 'bits + head': (no, yes, True),
       'acts + bits, no head': (yes, yes, False)}
  if depth >= 2:
    hole = [i != (depth // 2 if depth >= 3 else 0) for i in range(depth)]
    v['one layer with neither output'] = (hole, hole, True)
  return v


@pytest.mark.parametrize('W,K0,ld_feat,pad,depth,skip,M', [
    (128, 64, 64, 0, 1, 0, 256),        # one K step (only the stream's prologue), one layer, one tile
    (128, 192, 200, 8, 3, 1, 768),      # odd step count, padded strides, skip right after layer 0
    (256, 128, 128, 0, 8, 7, 512),      # maximum depth, skip into the last layer
    (256, 576, 576, 8, 2, 0, 256),      # long layer-0 stream (9 steps)
    (256, 64, 72, 0, 4, 2, 256),        # skip with the smallest feature segment
])
def test_chain_leaf_fwd(W, K0, ld_feat, pad, depth, skip, M):
  """mlp_chain_fwd_kernel: every layer, its 1-bit masks and the head against fp64; every output variant, the copy-out in
  front of the pass (mnr_mlp_chain_set_deferred(0)) and a capped grid bit for bit against the full default run."""
  inp = _leaf_fwd_inputs(W, K0, ld_feat, pad, depth, skip, M)
  yes = [True] * depth
  with _chain_switches() as sw:
    ref = _leaf_fwd_run(inp, yes, yes, True)
    ratios = _leaf_fwd_check(inp, ref)
    print(f'chain_leaf_fwd W={W} K0={K0} depth={depth} skip={skip} M={M}: worst error / bound per layer '
          + ' '.join(f'{r:.3f}' for r in ratios[:-1]) + f', head {ratios[-1]:.3f}')
    assert all(r <= 1.0 for r in ratios), ratios
    for a in ref['acts']:
      assert 0.2 < (a > 0).float().mean().item() < 0.8                 # (not a comparison of zeros)
    for defer in (1, 0):
      sw.set(defer=defer)
      if defer == 0:
        _leaf_same(ref, _leaf_fwd_run(inp, yes, yes, True), 'defer 0, everything')
      for name, (wa, wb, whd) in _leaf_fwd_variants(depth).items():
        _leaf_same(ref, _leaf_fwd_run(inp, wa, wb, whd), f'defer {defer}, {name}')
    if M > 256:                         # M = 768 on two workgroups: one walks two tiles, the other one
      sw.set(defer=1, max_wgs=2 if M == 768 else 1)
      _leaf_same(ref, _leaf_fwd_run(inp, yes, yes, True), 'capped grid')


def test_chain_leaf_fwd_edge_values():
  """Zeros and one non-finite feature: an output that is exactly zero (zero features and a zero bias of either sign, a unit
  with an all-zero weight row and zero bias) is the bit pattern 0x0000 with mask bit 0, and a +inf in one feature row touches
  no other row of the activations, masks or head."""
  W, K0, M = 128, 64, 256
  inp = _leaf_fwd_inputs(W, K0, K0, 0, 2, 0, M, seed=32)
  zrows = slice(32, 64)
  inp['feat'][zrows] = 0
  inp['bias'][0][0], inp['bias'][0][1] = 0.0, -0.0
  inp['Bt'][0][5], inp['bias'][0][5] = 0, 0.0
  inp['Bt'][1][7], inp['bias'][1][7] = 0, -0.0
  out = _leaf_fwd_run(inp, [True] * 2, [True] * 2, True)
  ratios = _leaf_fwd_check(inp, out)
  print('chain_leaf_fwd_edge_values: worst error / bound ' + ' '.join(f'{r:.3f}' for r in ratios))
  assert all(r <= 1.0 for r in ratios), ratios
  # zero features: layer 0 is relu(bias) rounded once, exactly
  want = torch.where(inp['bias'][0] > 0, inp['bias'][0], torch.zeros(())).to(_bf).expand(32, W)
  assert torch.equal(_i16(out['acts'][0][zrows]), _i16(want))
  m0, m1 = _unpack_mask(out['bits'][0], W), _unpack_mask(out['bits'][1], W)
  for what, a, m in (('zero bias', out['acts'][0][zrows, 0], m0[zrows, 0]), ('negative-zero bias', out['acts'][0][zrows, 1], m0[zrows, 1]),
                     ('zero unit of layer 0', out['acts'][0][:, 5], m0[:, 5]), ('zero unit of layer 1', out['acts'][1][:, 7], m1[:, 7])):
    assert bool((_i16(a) == 0).all()) and not bool(m.any()), what
  # row isolation
  row = 100
  inp['feat'][row, 3] = float('inf')
  bad = _leaf_fwd_run(inp, [True] * 2, [True] * 2, True)
  keep = torch.arange(M) != row
  for i in range(2):
    assert torch.equal(_i16(bad['acts'][i])[keep], _i16(out['acts'][i])[keep]), f'activation {i} outside the poisoned row'
    assert torch.equal(bad['bits'][i][keep], out['bits'][i][keep]), f'mask bits {i} outside the poisoned row'
  assert torch.equal(bad['head'].view(torch.int32)[keep], out['head'].view(torch.int32)[keep]), 'head outside the poisoned row'
  assert not bool(torch.isfinite(bad['acts'][0][row].float()).all())               # (the poison arrived)


def _leaf_masks(M, W, depth, g):
  """The test's own mask bytes (no forward pass): random, with all-zero and all-one rows, rows of single-bit bytes and rows
  with one single-bit byte, in the first and in the last tile."""
  out = []
  for i in range(depth):
    b = torch.randint(0, 256, (M, W // 8), generator=g, dtype=torch.uint8)
    for base in (0, M - 32):
      b[base], b[base + 1] = 0, 0xFF
      for e in range(8):
        b[base + 2 + e] = 1 << e
        b[base + 10 + e] = 0
        b[base + 10 + e, (3 * e + i) % (W // 8)] = 1 << e
    out.append(b)
  return out


def _leaf_bwd_run(W, M, masks, Bw, gh=None, wh=None, dY_in=None, store_last=True):
  ops = models.ops
  depth = len(masks)
  dY = [torch.full((M + 1, W), -_SENT, dtype=_bf, device='cuda') if (i < depth - 1 or store_last) else None for i in range(depth)]
  dev = lambda t: None if t is None else t.cuda()
  ops.mlp_chain_bwd(dev(gh), dev(wh), [b.cuda() for b in masks], [dev(w) for w in Bw], [None if d is None else d[:M] for d in dY],
                    M=M, W=W, dY_in=dev(dY_in))
  torch.cuda.synchronize()
  for d in dY:
    assert d is None or bool((d[M] == -_SENT).all()), 'dY guard row'
  return [None if d is None else d[:M].cpu().clone() for d in dY]


def _leaf_bwd_check(W, masks, Bw, dY, top):
  """dY[i - 1] against fp64 on the kernel's own dY[i] (`top` for the last layer) -> worst error / bound per layer, last first."""
  depth = len(masks)
  ratios = []
  for i in reversed(range(1, depth)):
    src = (top if i == depth - 1 else dY[i]).double()
    w = Bw[i][:, :W].double()
    z, mag = src @ w.T, src.abs() @ w.abs().T
    keep = _unpack_mask(masks[i - 1], W)
    got = dY[i - 1]
    ratios.append(_leaf_ratio(got, torch.where(keep, z, torch.zeros_like(z)), _leaf_bound(z, mag, W)))
    assert bool((_i16(got)[~keep] == 0).all()), f'dY[{i - 1}]: a masked element is not +0'
    # bit by bit: what is stored is non-zero exactly where the mask bit is set (and the fp64 value is not zero itself: rows
    # whose gradient or whose masks above are all zero)
    live = keep & (z.abs() > 1e-30)
    assert torch.equal(got != 0, live), f'dY[{i - 1}]: stored zeros and mask bits of layer {i - 1} disagree'
    assert live.float().mean().item() > 0.25
  return ratios


@pytest.mark.parametrize('W,depth,M', [(128, 1, 256), (128, 3, 768), (256, 8, 256), (256, 2, 768)])
def test_chain_leaf_bwd(W, depth, M):
  """mlp_chain_bwd_kernel on masks of the test's own: the rank-1 start bit for bit, every dX layer against fp64, masked elements
  exactly +0 and stored zeros agreeing with the mask bit by bit (bit order, byte order, which layer's masks are read); without
  dY[last], from dY_in, with the copy-out in front of the pass and on a capped grid bit for bit."""
  g = torch.Generator().manual_seed(41)
  masks = _leaf_masks(M, W, depth, g)
  Bw = [None]
  for i in range(1, depth):
    w = torch.full((W, W + 8), _NAN, dtype=_bf)
    w[:, :W] = ((torch.rand((W, W), generator=g) * 2 - 1) * (6.0 / W) ** 0.5).to(_bf)
    Bw.append(w)
  wh = (torch.rand((W,), generator=g) * 2 - 1) * 0.15
  gh = torch.randn((M,), generator=g) * 0.01
  gh[40:48] = torch.tensor([0.0, -0.0, 1e4, -1e4, 1e-20, -1e-20, 0.0, 1e4])
  gh[M - 48:M - 44] = torch.tensor([1e4, 1e-20, 0.0, -1e4])
  start = torch.where(_unpack_mask(masks[-1], W), (gh[:, None] * wh[None, :]).to(_bf), torch.zeros((), dtype=_bf))
  with _chain_switches() as sw:
    ref = _leaf_bwd_run(W, M, masks, Bw, gh, wh)
    assert torch.equal(_i16(ref[-1]), _i16(start)), 'rank-1 start: dY[last] is not bf16(fp32(g) fp32(w)) under the mask'
    ratios = _leaf_bwd_check(W, masks, Bw, ref, ref[-1])
    print(f'chain_leaf_bwd W={W} depth={depth} M={M}: worst error / bound per dX layer (last first) ' + ' '.join(f'{r:.3f}' for r in ratios))
    assert all(r <= 1.0 for r in ratios), ratios

    def same(got, what):
      for i, (x, y) in enumerate(zip(ref, got)):
        assert y is None or torch.equal(_i16(x), _i16(y)), f'{what}: dY[{i}]'

    same(_leaf_bwd_run(W, M, masks, Bw, gh, wh, store_last=False), 'without dY[last]')
    sw.set(defer=0)
    same(_leaf_bwd_run(W, M, masks, Bw, gh, wh), 'defer 0')
    same(_leaf_bwd_run(W, M, masks, Bw, gh, wh, store_last=False), 'defer 0 without dY[last]')
    if M > 256:
      sw.set(defer=1, max_wgs=2)
      same(_leaf_bwd_run(W, M, masks, Bw, gh, wh), 'capped grid')
    if (W, depth) in ((128, 3), (256, 2)):
      # the dY_in start (an MLP with heads; the Ref-NeRF tangent chain): a dY_last of the caller's
      sw.set()
      dy_in = torch.randn((M, W), generator=g).mul_(0.01).to(_bf)
      dy_in[40], dy_in[41] = 1e4, -1e-20
      ref_in = _leaf_bwd_run(W, M, masks, Bw, dY_in=dy_in, store_last=False)
      ratios = _leaf_bwd_check(W, masks, Bw, ref_in, dy_in)
      print(f'chain_leaf_bwd W={W} depth={depth} M={M} from dY_in: ' + ' '.join(f'{r:.3f}' for r in ratios))
      assert all(r <= 1.0 for r in ratios), ratios
      for defer, max_wgs in ((0, 0), (1, 2)):
        sw.set(defer=defer, max_wgs=max_wgs)
        got = _leaf_bwd_run(W, M, masks, Bw, dY_in=dy_in, store_last=False)
        for i in range(depth - 1):
          assert torch.equal(_i16(ref_in[i]), _i16(got[i])), f'dY_in start, defer {defer}, max_wgs {max_wgs}: dY[{i}]'


def _group_major_columns(K, L):
  """(source column of the [2KL] feature row / kernel row, group-major column) pairs of include/mnerf.h:
  column g*192 + dl*2K + s*K + k  =  kernel row s*K*L + (4g + dl)*K + k."""
  G = 192
  src, dst = [], []
  for gi in range(L // 4):
    for dl in range(4):
      for s in range(2):
        for k in range(K):
          src.append(s * K * L + (4 * gi + dl) * K + k)
          dst.append(gi * G + dl * 2 * K + s * K + k)
  return torch.tensor(src), torch.tensor(dst)


@pytest.mark.parametrize('K,min_deg,max_deg,W,n,B,ray_shape,contract,no_int', [
    (21, 0, 12, 256, 48, 16, 'cone', True, False),          # rays straddle the 256-row tiles
    (3, 0, 16, 128, 32, 8, 'cylinder', False, False),
    (3, 2, 6, 128, 32, 8, 'cone', True, False),             # non-zero min_deg, single group
    (24, 0, 8, 256, 64, 4, 'cone', False, False),           # no pad slots (8K = 192)
    (1, 0, 4, 128, 256, 1, 'cylinder', True, True),         # the lower edge of K; disable_integration
])
def test_chain_leaf_fwd_ipe(K, min_deg, max_deg, W, n, B, ray_shape, contract, no_int):
  """mlp_chain_fwd_ipe_kernel with a group-major Bt[0] the test builds itself from a row-major kernel: depth 1 against the fp64
  product of cast_rays_ipe's bf16 rows (pinned to the oracle by test_cast_rays_ipe), and depth 3 with its head bit for bit
  against mlp_chain_fwd on the feature matrix the test permutes into group-major order."""
  ops = models.ops
  L, M = max_deg - min_deg, B * n
  nfeat, ld_g = 2 * K * L, (L // 4) * 192
  g = torch.Generator().manual_seed(51)
  basis = torch.nn.functional.normalize(torch.randn((K, 3), generator=g), dim=-1).cuda()
  origins = (torch.randn((B, 3), generator=g) * 0.3).cuda()
  directions = torch.nn.functional.normalize(torch.randn((B, 3), generator=g), dim=-1).cuda() * 1.3
  radii = (0.002 + 0.002 * torch.rand((B,), generator=g)).cuda()
  tdist = torch.cumsum(0.02 + torch.rand((B, n + 1), generator=g) * (12.0 / n), dim=-1).cuda().contiguous()   # in and beyond the unit ball
  kw = dict(ray_shape=ray_shape, warp_contract=contract, min_deg=min_deg, max_deg=max_deg, disable_integration=no_int)
  kernel = ((torch.rand((nfeat, W), generator=g) * 2 - 1) * (6.0 / nfeat) ** 0.5).to(_bf)          # row-major: rows = inputs
  src, dst = _group_major_columns(K, L)
  Bt0 = torch.full((W, ld_g + 8), _NAN, dtype=_bf)
  Bt0[:, :ld_g] = 0
  Bt0[:, dst] = kernel.T[:, src]
  biases = [0.05 * torch.randn((W,), generator=g) for _ in range(3)]
  deeper = [((torch.rand((W, W), generator=g) * 2 - 1) * (6.0 / W) ** 0.5).to(_bf) for _ in range(2)]
  wh = ((torch.rand((W,), generator=g) * 2 - 1) * 0.15).to(_bf)
  bh = torch.full((1,), 0.0725)
  feat = ops.cast_rays_ipe(tdist, origins, directions, radii, basis, ld_feat=nfeat, **kw)
  # depth 1
  act = torch.full((M + 1, W), _SENT, dtype=_bf, device='cuda')
  ops.mlp_chain_fwd_ipe(tdist, origins, directions, radii, basis, [(Bt0.cuda(), biases[0].cuda())], M=M, W=W, act_last=act[:M], **kw)
  torch.cuda.synchronize()
  assert bool((act[M] == _SENT).all()), 'activation guard row'
  a, w, b = feat.cpu().double(), kernel.double(), biases[0].double()
  z, mag = a @ w + b, a.abs() @ w.abs() + b.abs()
  ratio = _leaf_ratio(act[:M].cpu(), z.clamp(min=0), _leaf_bound(z, mag, nfeat))
  print(f'chain_leaf_fwd_ipe K={K} degrees [{min_deg}, {max_deg}) W={W} n={n} {ray_shape}: layer 0 worst error / bound {ratio:.3f}')
  assert ratio <= 1.0
  assert 0.1 < (act[:M] > 0).float().mean().item() < 0.9 and a.abs().max().item() > 0.5
  # depth 3 with the head: the grouped route on the same bf16 features, the same operand, the same order over K
  feat_g = torch.zeros((M, ld_g), dtype=_bf)
  feat_g[:, dst] = feat.cpu()[:, src]
  layers = [(Bt0.cuda(), biases[0].cuda())] + [(deeper[i].cuda(), biases[i + 1].cuda()) for i in range(2)]
  outs = []
  for ipe in (True, False):
    x = torch.full((M + 1, W), _SENT, dtype=_bf, device='cuda')
    h = torch.full((M + 1,), _SENT, device='cuda')
    hk = dict(w_head=wh.cuda(), b_head=bh.cuda(), head_out=h[:M])
    if ipe:
      ops.mlp_chain_fwd_ipe(tdist, origins, directions, radii, basis, layers, M=M, W=W, act_last=x[:M], **hk, **kw)
    else:
      ops.mlp_chain_fwd(feat_g.cuda(), ld_g, layers, M=M, W=W, acts=[None, None, x[:M]], **hk)
    torch.cuda.synchronize()
    assert bool((x[M] == _SENT).all()) and h[M].item() == _SENT, 'guard row'
    outs.append((x[:M].cpu(), h[:M].cpu()))
  assert torch.equal(_i16(outs[0][0]), _i16(outs[1][0])), 'act_last: in-kernel IPE against the grouped feature matrix'
  assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)), 'head: in-kernel IPE against the grouped feature matrix'
  assert outs[0][1].abs().max().item() > 0 and bool(torch.isfinite(outs[0][1]).all())


def test_chain_leaf_rejects_bad_arguments():
  """One call per MNR_CHECK_ARG family of the three launchers, on the args structs themselves (ops.py's own assertions would
  intercept most of them): each raises with the launcher's message, and no output buffer is touched."""
  ops = models.ops
  Lb = ops.L
  lib = ops.lib()
  M, W, K0, n = 256, 128, 64, 32
  z = lambda shape, dt=_bf: torch.zeros(shape, dtype=dt, device='cuda')
  t = dict(feat=z((M, K0)), Bt0=z((W, 192)), Bt1=z((W, W + K0)), bias0=z((W + 4,), torch.float32), bias1=z((W,), torch.float32),
           wh=z((W,)), bh=z((1,), torch.float32), whf=z((W,), torch.float32), gh=z((M,), torch.float32), dY_in=z((M, W)),
           tdist=torch.linspace(0.1, 3.0, n + 1).repeat(M // n, 1).contiguous().cuda(), o=z((M // n, 3), torch.float32),
           d=torch.ones((M // n, 3)).cuda(), r=torch.full((M // n,), 0.01).cuda(), basis=torch.eye(3).cuda())
  outs = dict(acts0=z((M, W)), acts1=z((M, W)), bits0=z((M, W // 8), torch.uint8), bits1=z((M, W // 8), torch.uint8),
              head=z((M,), torch.float32), dY0=z((M, W)), dY1=z((M, W)))
  for o in outs.values():
    o.fill_(3)
  p = lambda x: x.data_ptr()

  def fwd():
    a = Lb.MlpChainFwdArgs()
    a.M, a.W, a.depth, a.skip_layer = M, W, 2, 0
    a.feat, a.ld_feat, a.K0 = p(t['feat']), K0, K0
    a.Bt[0], a.ldb[0], a.bias[0] = p(t['Bt0']), 192, p(t['bias0'])
    a.Bt[1], a.ldb[1], a.bias[1] = p(t['Bt1']), W + K0, p(t['bias1'])
    a.acts[0], a.acts[1], a.bits[0], a.bits[1] = p(outs['acts0']), p(outs['acts1']), p(outs['bits0']), p(outs['bits1'])
    a.w_head, a.b_head, a.head_out = p(t['wh']), p(t['bh']), p(outs['head'])
    return a

  def bwd():
    a = Lb.MlpChainBwdArgs()
    a.M, a.W, a.depth = M, W, 2
    a.g_head, a.w_head = p(t['gh']), p(t['whf'])
    a.bits[0], a.bits[1] = p(outs['bits0']), p(outs['bits1'])
    a.Bw[1], a.ldb[1] = p(t['Bt1']), W + K0
    a.dY[0], a.dY[1] = p(outs['dY0']), p(outs['dY1'])
    return a

  def ipe_chain():
    a = fwd()
    a.feat, a.ld_feat, a.K0 = None, 0, 0
    a.acts[0], a.bits[0], a.bits[1] = None, None, None
    return a

  def ipe_rays():
    q = Lb.ChainIpeArgs()
    q.cfg = Lb.IpeCfg(0, 1, 0, 3, 0, 4)
    q.n = n
    q.tdist, q.origins, q.directions, q.radii, q.basis = p(t['tdist']), p(t['o']), p(t['d']), p(t['r']), p(t['basis'])
    return q

  calls = {
      'mnr_mlp_chain_fwd': lambda a, q: lib.mnr_mlp_chain_fwd(C.byref(a), ops._stream()),
      'mnr_mlp_chain_bwd': lambda a, q: lib.mnr_mlp_chain_bwd(C.byref(a), ops._stream()),
      'mnr_mlp_chain_fwd_ipe': lambda a, q: lib.mnr_mlp_chain_fwd_ipe(C.byref(a), C.byref(q), ops._stream()),
  }
  make = {'mnr_mlp_chain_fwd': fwd, 'mnr_mlp_chain_bwd': bwd, 'mnr_mlp_chain_fwd_ipe': ipe_chain}

  def sa(**kv):                              # set fields; name_i addresses element i of an array field
    def mut(a, q):
      for k, v in kv.items():
        tgt, k = (q, k[2:]) if k.startswith('q_') else (a, k)
        el = re.fullmatch(r'(.+)_(\d)', k)
        if el:
          getattr(tgt, el.group(1))[int(el.group(2))] = v
        else:
          setattr(tgt, k, v)
    return mut

  def cfg(**kv):
    def mut(a, q):
      for k, v in kv.items():
        setattr(q.cfg, k, v)
    return mut

  cases = []
  for who in calls:                          # fm_check_common
    cases += [(who, sa(M=0), f'{who}: M=0 must be a positive multiple of 256'),
              (who, sa(M=255 + 1 - 2), f'{who}: M=254 must be a positive multiple of 256'),
              (who, sa(W=192), f'{who}: width 192 is not 128 or 256'),
              (who, sa(depth=0), f'{who}: depth 0 out of range'),
              (who, sa(depth=9), f'{who}: depth 9 out of range')]
  who = 'mnr_mlp_chain_fwd'
  cases += [(who, sa(K0=96), 'feature matrix needs K0'),
            (who, sa(ld_feat=K0 - 8), 'feature matrix needs K0'),
            (who, sa(skip_layer=1, ldb_1=W + K0 - 8), 'skip_layer 1 needs 0 < skip_layer < depth and an operand of W \\+ K0 columns'),
            (who, sa(skip_layer=2), 'skip_layer 2 needs 0 < skip_layer < depth'),
            (who, sa(bias_0=p(t['bias0'][1:])), 'bias\\[0\\] must be 16-byte aligned'),
            (who, sa(head_out=None), 'head needs head_out')]
  who = 'mnr_mlp_chain_bwd'
  cases += [(who, sa(dY_0=None), 'dY\\[0\\] missing'),
            (who, sa(dY_in=p(t['dY_in'])), 'with dY_in the last dY is the input itself'),
            (who, sa(bits_0=None), 'layer 0 needs its ReLU mask bits'),
            (who, sa(ldb_1=W - 8), 'layer 1 operand')]
  who = 'mnr_mlp_chain_fwd_ipe'
  cases += [(who, cfg(max_deg=6), 'degrees=6 \\(a multiple of 4\\) out of range'),
            (who, cfg(basis_k=25), 'basis_k=25 \\(1..24\\)'),
            (who, sa(skip_layer=1), 'no skip concat'),
            (who, sa(bits_1=p(outs['bits1'])), 'inference only'),
            (who, sa(q_n=48), 'M is not a whole number of rays'),
            (who, sa(w_head=None, acts_1=None), 'needs a head \\(with head_out\\) or acts\\[depth-1\\]')]
  for who, mut, msg in cases:
    a, q = make[who](), ipe_rays()
    mut(a, q)
    with pytest.raises(ValueError, match=msg):
      Lb.check(calls[who](a, q))
    torch.cuda.synchronize()
    for name, o in outs.items():
      assert bool((o == 3).all()), f'{who} ({msg}): touched {name}'
  # (the structs above are accepted as they stand: every rejection is the mutated field's)
  for who in calls:
    Lb.check(calls[who](make[who](), ipe_rays()))
  torch.cuda.synchronize()
