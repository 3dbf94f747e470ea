"""Leaf tests of the featurisation kernels against fp64 at free shapes.  -m gpu.

cast_rays_ipe_kernel in its three forms, cast_rays_ipe_bwd_kernel, cast_rays_ipe_tangent_bwd_kernel, the two
viewdir_enc_fill kernels and the GLO kernels (csrc/features.hip), ipe_from_gaussians_kernel (csrc/gaussians.hip), with what
they share (csrc/ipe_encode_body.inc, csrc/ipe_math.h), each against oracle/ in float64 (render.cast_rays,
coord.track_linearize(coord.contract), lift_and_diagonalize, integrated_pos_enc, pos_enc, autograd and
torch.autograd.functional.jvp) on inputs rounded to fp32 first.  The YARDSTICK is the same oracle in float32 on the same
inputs against the same fp64 values.  A kernel passes when

    figure <= MARGIN * yardstick,    MARGIN = 8 (tests/test_gpu_level_leaf.py)

The margin covers the device's sin and exp2 against the host's and the kernels' anchor-plus-recurrence evaluation of the
degrees.  FIGURES:
  * fp32 feature rows: per degree, the largest |got - ref64| over samples, directions and the sin / cos halves;
  * bf16 rows: bit-equal to the bf16 rounding of the fp32 rows where the fp32 entry accepts the shape (2KL % 4 == 0); and
    everywhere every entry within half a bf16 ulp + the fp32 bound of its degree; padding columns [2KL, ld_feat) exactly
    zero; the guard row behind every output untouched.  Half a bf16 ulp is 2^(e - 8) for a value in [2^e, 2^(e + 1)), taken
    at |ref64| + the fp32 bound (_half_ulp_bf16): between 2^-9 and 2^-8 of the value.  2^-9 |ref64| alone is the half ulp at
    the top of a binade only: at its foot the correctly rounded fp64 value itself is 2^-8 |ref64| away, and rows that ARE
    the rounded fp32 rows bit for bit read 1.93 against 2^-9 |ref64| + the fp32 bound (B = 15, n = 7, icosahedron 1);
  * tangent rows (bf16, three per sample): per degree against the fp64 JVP with the covariance held fixed, every entry
    within half a bf16 ulp + the bound of its degree;
  * post-warp means and covariances (want_gaussians): per sample, max |got - ref64| / max |ref64|, the worst sample;
  * gradients: g_t0 and g_t1 are added onto the ray's n + 1 interval ends in float64; per ray the largest |got - ref64|
    over the ends divided by the ray's largest |ref64|; the worst ray counts and no ray is left out.
FLOORS stand beside 8 x the yardstick only where derived from a count of roundings (an output that passes by a floor, its
error above 8 x the yardstick, is printed with a ^; a degree whose yardstick is above YARD_MAX is printed with a ~):
  * FLOOR_FWD = 160 x 2^-24 = 9.5e-6, absolute, on features of magnitude <= 1: the oracle's sin and exp of a degree are one
    library call each (half an ulp), while the kernels take sin, cos and exp2 at every fourth degree and reach the three
    degrees behind by recurrence.  The attenuation's exp2 is within 1 ulp (2 x 2^-24 relative at worst) and att(l+1) =
    att(l)^4 multiplies a relative error by 4 per step: 64 x 2 = 128.  The Cephes sin / cos are within ~1e-7 = 2 x 2^-24 and
    the double-angle step doubles an error and adds 1.5 roundings: 8 x 2 + (4 + 2 + 1) x 1.5 = 27, taken as 32.
  * FLOOR_ARG = 2 x 2^-24 x the largest |lm 2^l| of the case at that degree (lm = p_k . mean), added to FLOOR_FWD: the
    sine's argument is an fp32 number that no fp32 evaluation reaches through fewer than two roundings at its own magnitude
    (o + d t_mean and the projection; the scaling by 2^l is exact).  The oracle has them too, in the yardstick, and with
    many independent samples 8 x the yardstick is far above this (1e-2 at degree 15 in an ordinary scene); but ONE ray (B = 1)
    projected on an octahedron has one rounding error of the mean in common to all its samples, and the fp32 oracle's can be
    a fraction of an ulp by luck: tangent rows of B = 1, n = 83 at degree 15 read 0.74 for the oracle and 6.6 for the
    kernel at |T| = 1.2e4 (5.5e-4 of it, a quarter of an ulp of the argument 1.1e4).  At most 2e-4 at degree 15 in the
    small scene, beside 8 x a yardstick of 1e-4.
  * tangent rows: (256 x 2^-24 + FLOOR_ARG) x the largest |ref64| of the degree (the same 160, on both of att sin and att
    cos, which a tangent entry combines: x sqrt 2, taken as 256 / 160).
  * FLOOR_BWD = 680 x 2^-24 = 4.1e-5, relative to the ray's largest gradient: a gradient is a sum over the 2KL features of
    g x (scale) x (att cos, att sin), each carrying the 160 x 2^-24 above; independent errors add as a random walk, as do the
    terms of the sum itself (x sqrt 2 for the ratio of the two), and 3 standard deviations of that: 160 x 4.25.
  * FLOOR_GAUSS = 32 x 2^-24, relative per sample: the Gaussian is ~30 roundings deep in the kernels and in the oracle alike
    (t_mean 8, the lift 2, the contraction 10, the covariance's terms 10), and the two orders differ.
  * viewdir_enc_fill: 2 x 2^-24 (the device sinf within 2 ulp below 1; the identity columns are exact).
  * glo_bwd: (number of additions into the entry) x 2^-24 x the entry's largest partial sum.
YARD_MAX = 2e-4 keeps the yardstick honest: at degree l the fp32 oracle is off by |mean| 2^l 2^-24, 1e-2 at degree 15 in an
ordinary scene.  Every (entry point, degree 0..15) is therefore held in a `small scene` case (origins within 2^-5, unit
directions, radii 1e-6, tdist = 2^-6 + 8e-5 sorted uniform, octahedron, degrees [0, 16)) whose per-degree yardstick is at most
YARD_MAX (tangent rows: relative to 2^degree) and whose fp64 features reach 0.5 at that degree; both are asserted.  The VJPs are
held there ONE DEGREE AT A TIME (an upstream gradient that is zero outside the degree).  Degrees above the cap in the other
cases are still compared and printed.

The case tables are the smallest shapes that cross every boundary; the block sizes are the launchers' formulas restated
(_spb_fwd, _spb_bwd, SPB_TBWD), the totals B n are 1, spb - 1, spb, spb + 1 and 2 spb + 3 with an n that does not divide spb
where the total allows one.

Worst error / bound over the cases of each test (MI355X | kernel-source simulator):

  test                                   outputs
  fwd (rays)                             f32 0.35 | 0.28   bf16 0.99 | 0.99   means 0.12 | 0.12   covs 0.27 | 0.27
  tangent (rays)                         0.99 | 0.99
  small_scene_fwd                        f32 0.13 | 0.13   bf16 0.99 | 0.99   tangent 0.99 | 0.99
  bwd                                    two sources 0.27 | 0.22   one source 0.21 | 0.20
  tangent_bwd                            two sources 0.29 | 0.25   one source 0.24 | 0.24
  small_scene_bwd, worst degree          VJP 0.30 | 0.30   tangent VJP 0.23 | 0.23
  gaussians                              f32 0.34 | 0.31   bf16 0.99 | 0.99   means 0.09 | 0.09   covs 0.19 | 0.19
  gaussians_tangent                      0.99 | 0.99
  small_scene_gaussians                  f32 0.10 | 0.10   bf16 0.99 | 0.99   tangent 0.99 | 0.99   (means, covs: exact)
  edge_inputs                            f32 0.33 | 0.24   bf16 0.99 | 0.99   (the VJP: finite; its ratios, printed: <= 0.14)
  lds_refusal, ld_feat = 48              0.99 | 0.99
  viewdir_enc_fill                       1.00 | 1.00 (0.999)
  glo                                    0.20 | 0.20

The bf16 and tangent figures are the rounding to bf16 itself (half an ulp is most of their bound): what tells a wrong
kernel there is the bit-equality with the fp32 rows, which are held at 0.35, and the per-degree bound of the rest.  Every
bound was exercised on both the MI355X and the simulator.  ^ Outputs past 8 x the yardstick, inside a floor (degrees out of
~3,000 per-degree checks; MI355X | simulator): fp32 rows of rays 1 | 5, of Gaussians 10 | 7, tangent rows 1 | 1 (the B = 1
case above), gradients 1 | 1 (of ~260 checks).  The whole file takes 9 s on the MI355X and 25 s on the simulator on four workers.

Each of these, planted one at a time in a scratch copy, fails the tests named on the simulator: min_deg ignored in
cast_rays_ipe_bwd_kernel (35 cases of bwd) or in cast_rays_ipe_tangent_bwd_kernel (16 of tangent_bwd); att(l+1) = att(l)^2
(every family of rows and both VJPs); the anchor every 8th degree (fwd, tangent, gaussians, edge_inputs); the padding loop
from 2KL + 1 (every family of rows); one row too many in the write-out (the guard rows); the sin / cos halves of the
element-wise viewdir_enc_fill_kernel swapped (24 cases); g_feat_b ignored (all 50 of bwd); the off-diagonal weights of the
covariance gradient set to 1 (30 of bwd).
"""

import ctypes as C
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import coord as ocoord
from oracle import render as orender
from tests.test_gpu_level_leaf import MARGIN, U, YARD_MAX

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16

FLOOR_FWD = 160 * U
FLOOR_TAN = 256 * U            # x the degree's largest |ref64|
FLOOR_ARG = 2 * U              # x the largest |sine argument| of the degree (x the degree's largest |ref64| for tangent rows)
FLOOR_BWD = 680 * U
FLOOR_GAUSS = 32 * U
FLOOR_VIEW = 2 * U
SENT = 7.0


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from multinerf_amd import ops as _ops
  _ops.lib()
  return _ops


def dev(x):
  return None if x is None else x.contiguous().cuda()


# ----------------------------------------------------------------------------- block sizes: the launchers' formulas

SPB_TBWD = 32                                                   # FE_TB_SPB


def _spb_fwd(row_elems, f32_rows=False, tangent=False):
  """fe_block_geometry: row_elems = ld_feat for bf16 rows, 2KL for fp32 rows."""
  row_bytes = row_elems * (4 if f32_rows else 2)
  return min(256, 32768 // (row_bytes * (3 if tangent else 1))) & ~3


def _lds_fwd(row_elems, K, tangent):
  spb = _spb_fwd(row_elems, tangent=tangent)
  return spb * (36 + (108 if tangent else 0)) + ((K * 3 + 3) & ~3) * 4 + spb * (2 * row_elems + 48) * (3 if tangent else 1)


def _spb_bwd(K, L):
  return min(64, 40960 // (4 * ((2 * K * L) | 1) + 8 * K)) & ~3


def _totals(spb):
  return [1, spb - 1, spb, spb + 1, 2 * spb + 3]


def _split(T, spb, k):
  """T = B n with an n that does not divide spb (blocks straddle rays) where T has such a factor; else B = 1 or n = 1."""
  for n in (7, 5, 37, 3, 11, 13):
    if T % n == 0 and T > n and spb % n != 0:
      return T // n, n
  return (1, T) if k % 2 == 0 else (T, 1)


# ----------------------------------------------------------------------------- configurations

DEGS = [(0, 16), (0, 12), (2, 7), (3, 12), (1, 2), (5, 6), (4, 12), (1, 8)]       # L = 16, 12, 5, 9, 1, 1, 8 and 7
BASES = {'unit1': 1, 'octa1': 3, 'ico1': 6, 'ico2': 21, 'ico3': 46}
LD_KINDS = ('up8', 'up8+8', 'up128')
#        basis    degrees  ld_feat   ray shape   contract  disable_integration
CFGS = [('octa1', (0, 16), 'up128', 'cone', False, False),
        ('unit1', (0, 16), 'up8', 'cylinder', True, False),
        ('ico1', (0, 12), 'up8+8', 'cone', True, False),
        ('ico2', (2, 7), 'up8', 'cylinder', False, False),          # 2KL = 210: no fp32 rows
        ('ico3', (3, 12), 'up8', 'cone', True, False),              # 46 directions: several passes of the pair loop
        ('octa1', (1, 2), 'up8+8', 'cone', False, True),            # 2KL = 6
        ('ico1', (5, 6), 'up128', 'cylinder', True, True),
        ('ico2', (4, 12), 'up128', 'cone', True, False),
        ('unit1', (3, 12), 'up8+8', 'cone', False, False),          # 2KL = 18
        ('octa1', (1, 8), 'up8', 'cylinder', False, False)]         # L = 7
TBWD_CFGS = [0, 1, 2, 5, 6, 8]                                      # the tangent VJP's reference is reverse over forward: K <= 6
TBWD_K21 = (3, 33)                                                  # ... plus one case at K = 21: (configuration, total)


@functools.lru_cache(maxsize=None)
def _basis(name):
  """[K, 3] fp32 (shared between the cases: never written to)."""
  from multinerf_amd import geopoly
  if name == 'unit1':
    return torch.tensor([[0.6, -0.48, 0.64]], dtype=f32)           # a hand-made unit vector
  shape, v = {'octa1': ('octahedron', 1), 'ico1': ('icosahedron', 1), 'ico2': ('icosahedron', 2), 'ico3': ('icosahedron', 3)}[name]
  P = torch.as_tensor(geopoly.generate_basis(shape, v), dtype=f32)
  assert P.shape == (BASES[name], 3)
  return P


def _ld(F, kind):
  up8 = (F + 7) // 8 * 8
  return {'up8': up8, 'up8+8': up8 + 8, 'up128': (F + 127) // 128 * 128}[kind]


def _cfg(row, ld_min=0):
  basis, (lo, hi), kind, shape, contract, no_int = row
  P = _basis(basis)
  K, L = P.shape[0], hi - lo
  F = 2 * K * L
  ld = _ld(F, kind)
  if ld < ld_min:
    ld = _ld(F, 'up128')
  return dict(P=P, K=K, L=L, F=F, ld=ld, min_deg=lo, max_deg=hi, shape=shape, contract=contract, no_int=no_int,
              id=f'{basis}-deg{lo}_{hi}-ld{ld}-{shape}-{"contract" if contract else "nowarp"}{"-noint" if no_int else ""}')


def _kw(cfg):
  return dict(ray_shape=cfg['shape'], warp_contract=cfg['contract'], min_deg=cfg['min_deg'], max_deg=cfg['max_deg'],
              disable_integration=cfg['no_int'])


def test_ipe_leaf_config_table_covers_every_value():
  """Every basis, degree range, ld_feat kind, ray shape with the contraction on and off, disable_integration on (with and
  without the contraction); L of 1, 4k and 4k +- 1; a non-zero min_deg in every entry point's table, both VJPs included; a
  feature count that the fp32 rows refuse."""
  assert {r[0] for r in CFGS} == set(BASES) and {r[1] for r in CFGS} == set(DEGS) and {r[2] for r in CFGS} == set(LD_KINDS)
  assert {(r[3], r[4]) for r in CFGS} == {(s, c) for s in ('cone', 'cylinder') for c in (True, False)}
  assert {r[4] for r in CFGS if r[5]} == {True, False}
  Ls = {hi - lo for _, (lo, hi), *_ in CFGS}
  assert 1 in Ls and any(l % 4 == 0 for l in Ls) and any(l % 4 == 1 and l > 1 for l in Ls) and any(l % 4 == 3 for l in Ls)
  assert any((2 * BASES[r[0]] * (r[1][1] - r[1][0])) % 4 for r in CFGS)
  tb = [CFGS[i] for i in TBWD_CFGS] + [CFGS[TBWD_K21[0]]]
  assert any(r[1][0] > 0 for r in tb) and any(r[5] for r in tb) and all(BASES[CFGS[i][0]] <= 6 for i in TBWD_CFGS)
  assert BASES[CFGS[TBWD_K21[0]][0]] == 21
  assert any(16 * BASES[r[0]] > 256 for r in CFGS)                 # more than one pass of the (sample, direction) loop


# ----------------------------------------------------------------------------- inputs


def _rays(seed, B, n, kind='mid', radius_scale=1.0):
  """'mid': origins within 0.6 of the centre, |d| in [0.8, 1.2], t in [0.05, 2.55]: means on both sides of |x| = 1.
  'small': the small scene of the module docstring."""
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.rand(s, generator=g, dtype=f64)
  d = torch.randn((B, 3), generator=g, dtype=f64)
  d = d / d.norm(dim=-1, keepdim=True)
  if kind == 'small':
    o = (r(B, 3) * 2 - 1) * 2.0 ** -5
    radii = torch.full((B,), 1e-6, dtype=f64)
    tdist = 2.0 ** -6 + 8e-5 * torch.sort(r(B, n + 1), -1).values
  else:
    o = (r(B, 3) * 2 - 1) * 0.6
    d = d * (0.8 + 0.4 * r(B, 1))
    radii = (3e-4 + 7e-4 * r(B)) * radius_scale
    tdist = 0.05 + 2.5 * torch.sort(r(B, n + 1), -1).values
  return dict(B=B, n=n, o=o.float(), d=d.float(), radii=radii.float(), tdist=tdist.float())


def _dev_rays(inp):
  return tuple(dev(inp[k]) for k in ('tdist', 'o', 'd', 'radii'))


def _upstream(seed, rows, cfg, ld, power, degree=None):
  """bf16 upstream gradient [rows, ld]: N(0, 1) 2^(-power l) in the column of degree l (the features' derivatives grow like
  2^l, the tangent rows' like 4^l), zero outside `degree` if one is given, and N(0, 1) in the padding columns [2KL, ld),
  which no kernel may read."""
  g = torch.Generator().manual_seed(seed)
  K, L, F = cfg['K'], cfg['L'], cfg['F']
  deg = torch.arange(L).repeat_interleave(K).repeat(2)
  scale = 2.0 ** (-float(power) * (deg + cfg['min_deg']).double())
  if degree is not None:
    scale = scale * (deg == degree)
  x = torch.randn((rows, ld), generator=g, dtype=f64)
  x[:, :F] *= scale
  return x.to(bf16)


# ----------------------------------------------------------------------------- the reference: oracle/ in `dtype`


def _ref_gaussians(cfg, inp, dtype, t=None):
  """-> (pre-warp means, pre-warp covs, post-warp means, post-warp covs), [B, n, ...]."""
  c = lambda x: x.to(dtype)
  t = c(inp['tdist']) if t is None else t
  m0, c0 = orender.cast_rays(t, c(inp['o']), c(inp['d']), c(inp['radii'])[:, None], cfg['shape'], diag=False)
  if cfg['no_int']:
    c0 = torch.zeros_like(c0)
  m1, c1 = ocoord.track_linearize(ocoord.contract, m0, c0) if cfg['contract'] else (m0, c0)
  return m0, c0, m1, c1


def _encode(cfg, means, covs):
  lm, lv = ocoord.lift_and_diagonalize(means, covs, cfg['P'].to(means.dtype).t())
  return ocoord.integrated_pos_enc(lm, lv, cfg['min_deg'], cfg['max_deg']).reshape(-1, cfg['F'])


def _tangent_rows(cfg, m0, c0, create_graph=False):
  """d features / d (pre-warp mean)_c, c = x, y, z, the covariance held fixed and the contraction inside: [3 M, 2KL]."""
  def feat_of(mu):
    m1, c1 = ocoord.track_linearize(ocoord.contract, mu, c0) if cfg['contract'] else (mu, c0)
    return _encode(cfg, m1, c1)
  rows = []
  for c in range(3):
    e = torch.zeros_like(m0)
    e[..., c] = 1.0
    rows.append(torch.autograd.functional.jvp(feat_of, m0, e, create_graph=create_graph)[1])
  return torch.cat(rows, 0)


def _ref_rows(cfg, inp, dtype, tangent=False):
  m0, c0, m1, c1 = _ref_gaussians(cfg, inp, dtype)
  return _tangent_rows(cfg, m0, c0) if tangent else _encode(cfg, m1, c1)


def _ray_arg(cfg, inp):
  return _arg_max(cfg, _ref_gaussians(cfg, inp, f64)[2])


def _ref_grad(cfg, inp, dtype, G, tangent=False):
  """d <G, rows> / d tdist, [B, n + 1]; G: the upstream gradient the kernel is given, as float64."""
  t = inp['tdist'].to(dtype).clone().requires_grad_(True)
  m0, c0, m1, c1 = _ref_gaussians(cfg, inp, dtype, t)
  rows = _tangent_rows(cfg, m0, c0, create_graph=True) if tangent else _encode(cfg, m1, c1)
  (rows * G[:, :cfg['F']].to(dtype)).sum().backward()
  return t.grad.detach()


# ----------------------------------------------------------------------------- figures and bounds


def _ratio(fig, bound):
  return fig / bound if bound > 0 else (0.0 if fig == 0 else math.inf)


def _deg_max(x, cfg):
  """[rows, 2KL] -> [L]: the largest magnitude per degree over rows, directions and the sin / cos halves."""
  return torch.nan_to_num(x.double().abs(), nan=math.inf).reshape(x.shape[0], 2, cfg['L'], cfg['K']).amax((0, 1, 3))


def _deg_cols(v, cfg):
  """[L] -> [2KL]: a per-degree value for every column."""
  return v.repeat_interleave(cfg['K']).repeat(2)


def _half_ulp_bf16(ref, slack):
  """Half a bf16 ulp of any value within `slack` of `ref`: 2^(e - 8) with 2^e <= |ref| + slack < 2^(e + 1).  Between 2^-9 and
  2^-8 of the value: 2^-9 |ref| is the half ulp at the TOP of a binade only; at its foot the correctly rounded fp64 value
  itself is up to 2^-8 |ref| away."""
  x = (ref.abs() + slack).clamp(min=2.0 ** -126)
  return 2.0 ** (torch.floor(torch.log2(x)) - 8)


def _arg_max(cfg, means):
  """[L]: the largest |lm 2^degree| of the case, lm = p_k . (post-warp mean): the magnitude of the sine's argument."""
  lm = (means.double().reshape(-1, 3) @ cfg['P'].double().t()).abs().max()
  return lm * 2.0 ** (torch.arange(cfg['L']) + cfg['min_deg']).double()


def _hold_rows(label, cfg, got, r64, r32, floor, arg, half_ulp=False, scale_floor=False):
  """Per degree.  fp32 rows: max |got - ref64| <= max(8 yardstick, floor + FLOOR_ARG arg).  half_ulp (bf16 rows): every entry
  within half a bf16 ulp + that bound.  scale_floor: the floor is relative to the degree's largest |ref64|.  Prints the ratios
  (^: past 8 x the yardstick, by the floor; ~: the yardstick is above YARD_MAX), asserts, returns (worst ratio, yardsticks)."""
  got, r64, r32 = got.double().cpu(), r64.double(), r32.double()
  assert torch.isfinite(r64).all(), 'the fp64 reference must be finite'
  yard = _deg_max(r32 - r64, cfg)
  fl = (floor + FLOOR_ARG * arg) * (_deg_max(r64, cfg) if scale_floor else 1.0)
  bound = torch.maximum(MARGIN * yard, fl)
  err = torch.nan_to_num((got - r64).abs(), nan=math.inf)
  if half_ulp:
    ratio = _deg_max(err / (_half_ulp_bf16(r64, _deg_cols(bound, cfg)) + _deg_cols(bound, cfg)).clamp(min=1e-300), cfg)
    y8 = _deg_cols(MARGIN * yard, cfg)
    by_floor = _deg_max(err / (_half_ulp_bf16(r64, y8) + y8).clamp(min=1e-300), cfg) > 1
  else:
    e = _deg_max(err, cfg)
    ratio = torch.where(bound > 0, e / bound.clamp(min=1e-300), torch.where(e > 0, torch.full_like(e, math.inf), torch.zeros_like(e)))
    by_floor = _deg_max(err, cfg) > MARGIN * yard
  scale = 2.0 ** (torch.arange(cfg['L']) + cfg['min_deg']).double() if scale_floor else 1.0
  marks = ['^' * bool(by_floor[l]) + '~' * bool((yard / scale)[l] > YARD_MAX) for l in range(cfg['L'])]
  print(f'{label}: worst {ratio.max().item():.3f}; per degree ' + ' '.join(f'{ratio[l].item():.2f}{marks[l]}' for l in range(cfg['L'])))
  bad = [f'degree {cfg["min_deg"] + l}: error / bound {ratio[l].item():.3f} (bound {bound[l].item():.3e}, fp32 oracle {yard[l].item():.3e})'
         for l in range(cfg['L']) if not ratio[l] <= 1.0]
  assert not bad, f'{label}: ' + '; '.join(bad)
  return ratio.max().item(), yard


def _ray_figure(got, ref):
  """Worst ray's max |got - ref| / max |ref|.  A ray that is all zero in fp64 is measured at the batch's scale."""
  got, ref = got.double().cpu().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
  assert torch.isfinite(ref).all(), 'the fp64 reference must be finite'
  scale = ref.abs().amax(1)
  scale = torch.where(scale > 0, scale, scale.max())
  err = torch.nan_to_num((got - ref).abs(), nan=math.inf).amax(1)
  fig = torch.where(scale > 0, err / scale.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
  return fig.max().item()


def _hold_rays(label, items):
  """items: (name, got, ref64, ref32, floor): per-row relative figures; prints, asserts, returns {name: (ratio, yardstick)}."""
  parts, bad, out = [], [], {}
  for name, got, r64, r32, floor in items:
    fig, yard = _ray_figure(got, r64), _ray_figure(r32, r64)
    bound = max(MARGIN * yard, floor)
    ratio = _ratio(fig, bound)
    out[name] = (ratio, yard)
    parts.append(f'{name} {ratio:.3f}' + ('^' if fig > MARGIN * yard else '') + ('~' if yard > YARD_MAX else ''))
    if not ratio <= 1.0:
      bad.append(f'{name}: error {fig:.3e} > bound {bound:.3e} (fp32 oracle {yard:.3e})')
  print(f'{label}: worst error / bound ' + ' '.join(parts))
  assert not bad, f'{label}: ' + '; '.join(bad)
  return out


def _assert_coverage(label, cfg, yard, r64, scale=None):
  """The small scene holds every degree 0..15 under YARD_MAX with fp64 features that reach 0.5."""
  assert (cfg['min_deg'], cfg['max_deg']) == (0, 16)
  y = yard if scale is None else yard / scale
  amp = _deg_max(r64, cfg)
  assert (y <= YARD_MAX).all(), f'{label}: yardstick above YARD_MAX: {y.tolist()}'
  assert (amp >= 0.5).all(), f'{label}: fp64 features below 0.5: {amp.tolist()}'


# ----------------------------------------------------------------------------- kernel calls, with a guard row behind every output


def _guarded(rows, cols, dtype, fill=SENT):
  buf = torch.full((rows + 1, cols), fill, dtype=dtype).cuda()
  return buf, buf[:rows]


def _guard_ok(buf, fill=SENT):
  return bool((buf[-1].float().cpu() == fill).all())


def _kernel_fwd(ops, cfg, inp, f32_rows=False):
  """mnr_cast_rays_ipe with want_gaussians (bf16 rows, means, covs) or mnr_cast_rays_ipe_f32, through the C ABI so that every
  output has a guard row."""
  M = inp['B'] * inp['n']
  c = ops._ipe_cfg(cfg['shape'], cfg['contract'], cfg['no_int'], cfg['P'], cfg['min_deg'], cfg['max_deg'])
  a = _dev_rays(inp) + (dev(cfg['P']),)
  p = [ops._ptr(x) for x in a]
  if f32_rows:
    buf, out = _guarded(M, cfg['F'], f32)
    ops.L.check(ops.lib().mnr_cast_rays_ipe_f32(C.byref(c), inp['B'], inp['n'], *p, ops._ptr(out), ops._stream()))
    torch.cuda.synchronize()
    assert _guard_ok(buf), 'fp32 rows: guard row'
    return out
  buf, out = _guarded(M, cfg['ld'], bf16)
  mb, means = _guarded(M, 3, f32)
  cb, covs = _guarded(M, 9, f32)
  ops.L.check(ops.lib().mnr_cast_rays_ipe(C.byref(c), inp['B'], inp['n'], *p, ops._ptr(out), cfg['ld'], ops._ptr(means), ops._ptr(covs),
                                          ops._stream()))
  torch.cuda.synchronize()
  assert _guard_ok(buf) and _guard_ok(mb) and _guard_ok(cb), 'bf16 rows / means / covs: guard row'
  return out, means, covs


def _check_bf16(label, cfg, rows, rows32, r64, r32, arg, floor=FLOOR_FWD, scale_floor=False):
  """bf16 rows [*, ld]: the padding columns exactly zero; bit-equal to the rounded fp32 rows where there are any, and within
  half a bf16 ulp plus the fp32 bound of the fp64 reference."""
  F = cfg['F']
  rows = rows.cpu()
  assert not rows[:, F:].float().abs().any(), f'{label}: padding columns [2KL, ld_feat) are not zero'
  if rows32 is not None:
    assert torch.equal(rows[:, :F], rows32.cpu().to(bf16)), f'{label}: bf16 rows are not the rounded fp32 rows'
  return _hold_rows(label, cfg, rows[:, :F].float(), r64, r32, floor, arg, half_ulp=True, scale_floor=scale_floor)


# ----------------------------------------------------------------------------- forward: rays


def _fwd_cases():
  out = []
  for ci, row in enumerate(CFGS):
    cfg = _cfg(row)
    Ts = set(_totals(_spb_fwd(cfg['ld'])))
    if cfg['F'] % 4 == 0:
      Ts |= set(_totals(_spb_fwd(cfg['F'], f32_rows=True)))
    out += [(ci, T) for T in sorted(Ts)]
  return out


def _tan_cases():
  return [(ci, T) for ci, row in enumerate(CFGS) for T in _totals(_spb_fwd(_cfg(row, 48)['ld'], tangent=True))]


def _assert_totals_cross(cases, spb_of, label, split_spb_of=None):
  """Each configuration runs totals of 1, spb - 1, spb, spb + 1 and 2 spb + 3 of its own block size; over the table B = 1,
  n = 1 and multi-block totals with an n that does not divide spb all occur."""
  shapes = []
  for ci in sorted({c for c, _ in cases}):
    spb = spb_of(ci)
    assert spb >= 4
    Ts = [T for c, T in cases if c == ci]
    assert set(_totals(spb)) <= set(Ts), (label, ci, spb, Ts)
    shapes += [(T, spb) + _split(T, (split_spb_of or spb_of)(ci), k) for k, T in enumerate(Ts)]     # (the shapes the tests run)
  assert any(B == 1 and n > 1 for T, spb, B, n in shapes) and any(n == 1 and B > 1 for T, spb, B, n in shapes)
  assert any(T == 1 for T, *_ in shapes)
  assert any(T > spb and spb % n != 0 and n > 1 and B > 1 for T, spb, B, n in shapes), f'{label}: no block straddles a ray'


def test_ipe_leaf_fwd_table_covers_every_value():
  _assert_totals_cross(_fwd_cases(), lambda ci: _spb_fwd(_cfg(CFGS[ci])['ld']), 'bf16 rows')
  f32_cfgs = [ci for ci, r in enumerate(CFGS) if _cfg(r)['F'] % 4 == 0]
  _assert_totals_cross([c for c in _fwd_cases() if c[0] in f32_cfgs], lambda ci: _spb_fwd(_cfg(CFGS[ci])['F'], f32_rows=True), 'fp32 rows',
                       lambda ci: _spb_fwd(_cfg(CFGS[ci])['ld']))
  _assert_totals_cross(_tan_cases(), lambda ci: _spb_fwd(_cfg(CFGS[ci], 48)['ld'], tangent=True), 'tangent rows')
  assert {_spb_fwd(_cfg(r)['ld']) for r in CFGS} >= {256} and min(_spb_fwd(_cfg(r)['ld']) for r in CFGS) < 32   # capped by the threads / by LDS
  for r in CFGS:
    c = _cfg(r, 48)
    assert _lds_fwd(c['ld'], c['K'], True) <= 65536


def _case_inputs(cases, case, spb, seed):
  ci, T = case
  k = [t for c, t in cases if c == ci].index(T)
  B, n = _split(T, spb, k)
  return _rays(seed + 100 * ci + k, B, n)


def _both_sides(cfg, r64_pre_means):
  m = (r64_pre_means ** 2).sum(-1)
  return bool((m > 1).any() and (m < 1).any())


@pytest.mark.parametrize('case', _fwd_cases(), ids=lambda c: f'{_cfg(CFGS[c[0]])["id"]}-T{c[1]}')
def test_ipe_leaf_fwd(ops, case):
  """mnr_cast_rays_ipe with want_gaussians and mnr_cast_rays_ipe_f32."""
  cfg = _cfg(CFGS[case[0]])
  inp = _case_inputs(_fwd_cases(), case, _spb_fwd(cfg['ld']), 1000)
  g64, g32 = _ref_gaussians(cfg, inp, f64), _ref_gaussians(cfg, inp, f32)
  r64, r32 = _encode(cfg, g64[2], g64[3]), _encode(cfg, g32[2], g32[3])
  if cfg['contract'] and case[1] >= 16:
    assert _both_sides(cfg, g64[0]), 'the contracted cases have samples on both sides of |x| = 1'
  label = f'ipe_leaf_fwd {cfg["id"]} B={inp["B"]} n={inp["n"]}'
  arg = _arg_max(cfg, g64[2])
  rows32 = None
  if cfg['F'] % 4 == 0:
    rows32 = _kernel_fwd(ops, cfg, inp, f32_rows=True)
    _hold_rows(label + ' f32', cfg, rows32, r64, r32, FLOOR_FWD, arg)
  rows, means, covs = _kernel_fwd(ops, cfg, inp)
  _check_bf16(label + ' bf16', cfg, rows, rows32, r64, r32, arg)
  _hold_rays(label, [('means', means, g64[2].reshape(-1, 3), g32[2].reshape(-1, 3), FLOOR_GAUSS),
                     ('covs', covs, g64[3].reshape(-1, 9), g32[3].reshape(-1, 9), FLOOR_GAUSS)])


@pytest.mark.parametrize('case', _tan_cases(), ids=lambda c: f'{_cfg(CFGS[c[0]], 48)["id"]}-T{c[1]}')
def test_ipe_leaf_tangent(ops, case):
  """mnr_cast_rays_ipe_tangent (ld_feat >= 48: shorter rows are refused, test_ipe_leaf_lds_refusal)."""
  cfg = _cfg(CFGS[case[0]], 48)
  inp = _case_inputs(_tan_cases(), case, _spb_fwd(cfg['ld'], tangent=True), 2000)
  M = inp['B'] * inp['n']
  r64, r32 = _ref_rows(cfg, inp, f64, True), _ref_rows(cfg, inp, f32, True)
  buf, out = _guarded(3 * M, cfg['ld'], bf16)
  ops.cast_rays_ipe_tangent(*_dev_rays(inp), dev(cfg['P']), ld_feat=cfg['ld'], out=out, **_kw(cfg))
  torch.cuda.synchronize()
  assert _guard_ok(buf), 'tangent rows: guard row'
  _check_bf16(f'ipe_leaf_tangent {cfg["id"]} B={inp["B"]} n={inp["n"]}', cfg, out, None, r64, r32, _ray_arg(cfg, inp), FLOOR_TAN, scale_floor=True)


SMALL_ROW = ('octa1', (0, 16), 'up128', None, None, False)


def _small_cfg(shape, contract):
  return _cfg(SMALL_ROW[:3] + (shape, contract, False))


SMALL_VARIANTS = [('cone', False), ('cylinder', False), ('cone', True)]


@pytest.mark.parametrize('shape,contract', SMALL_VARIANTS)
def test_ipe_leaf_small_scene_fwd(ops, shape, contract):
  """The small scene: every degree 0..15 of the bf16, fp32 and tangent rows under YARD_MAX at an amplitude of 0.5 or more."""
  cfg = _small_cfg(shape, contract)
  inp = _rays(31, 7, 5, 'small')
  r64, r32 = _ref_rows(cfg, inp, f64), _ref_rows(cfg, inp, f32)
  label = f'ipe_leaf_small_scene_fwd {shape} contract={contract}'
  rows32 = _kernel_fwd(ops, cfg, inp, f32_rows=True)
  arg = _ray_arg(cfg, inp)
  _, yard = _hold_rows(label + ' f32', cfg, rows32, r64, r32, FLOOR_FWD, arg)
  _assert_coverage(label, cfg, yard, r64)
  rows, _, _ = _kernel_fwd(ops, cfg, inp)
  _check_bf16(label + ' bf16', cfg, rows, rows32, r64, r32, arg)
  t64, t32 = _ref_rows(cfg, inp, f64, True), _ref_rows(cfg, inp, f32, True)
  buf, out = _guarded(3 * 35, cfg['ld'], bf16)
  ops.cast_rays_ipe_tangent(*_dev_rays(inp), dev(cfg['P']), ld_feat=cfg['ld'], out=out, **_kw(cfg))
  torch.cuda.synchronize()
  assert _guard_ok(buf)
  _, yard_t = _check_bf16(label + ' tangent', cfg, out, None, t64, t32, arg, FLOOR_TAN, scale_floor=True)
  _assert_coverage(label + ' tangent', cfg, yard_t, r64, scale=2.0 ** torch.arange(16).double())


# ----------------------------------------------------------------------------- the VJPs


def _fence(B, n, a0, a1):
  """Per-sample (d / d t0, d / d t1) -> per interval end, in float64: [B, n + 1]."""
  out = torch.zeros((B, n + 1), dtype=f64)
  out[:, :n] += a0.double().cpu().reshape(B, n)
  out[:, 1:] += a1.double().cpu().reshape(B, n)
  return out


def _kernel_bwd(ops, cfg, inp, gA, gB):
  M = inp['B'] * inp['n']
  b0, g0 = _guarded(M, 1, f32, math.nan)
  b1, g1 = _guarded(M, 1, f32, math.nan)
  ops.cast_rays_ipe_bwd(*_dev_rays(inp), dev(cfg['P']), dev(gA), dev(gB), g_t0=g0.view(-1), g_t1=g1.view(-1), **_kw(cfg))
  torch.cuda.synchronize()
  assert bool(torch.isnan(b0[-1]).all() and torch.isnan(b1[-1]).all()), 'g_t0 / g_t1: guard element'
  return _fence(inp['B'], inp['n'], g0, g1)


def _kernel_tbwd(ops, cfg, inp, gA, gB, init0, init1):
  """Accumulates onto (init0, init1)."""
  M = inp['B'] * inp['n']
  b0, g0 = _guarded(M, 1, f32, math.nan)
  b1, g1 = _guarded(M, 1, f32, math.nan)
  g0.view(-1).copy_(init0)
  g1.view(-1).copy_(init1)
  ops.cast_rays_ipe_tangent_bwd(*_dev_rays(inp), dev(cfg['P']), dev(gA), dev(gB), g0.view(-1), g1.view(-1), **_kw(cfg))
  torch.cuda.synchronize()
  assert bool(torch.isnan(b0[-1]).all() and torch.isnan(b1[-1]).all()), 'g_t0 / g_t1: guard element'
  return _fence(inp['B'], inp['n'], g0, g1)


def _bwd_cases():
  return [(ci, T) for ci, row in enumerate(CFGS) for T in _totals(_spb_bwd(BASES[row[0]], row[1][1] - row[1][0]))]


def _tbwd_cases():
  return [(ci, T) for ci in TBWD_CFGS for T in _totals(SPB_TBWD)] + [TBWD_K21]


def test_ipe_leaf_bwd_table_covers_every_value():
  _assert_totals_cross(_bwd_cases(), lambda ci: _spb_bwd(BASES[CFGS[ci][0]], CFGS[ci][1][1] - CFGS[ci][1][0]), 'bwd')
  _assert_totals_cross([c for c in _tbwd_cases() if c != TBWD_K21], lambda ci: SPB_TBWD, 'tangent bwd')
  spbs = {_spb_bwd(BASES[r[0]], r[1][1] - r[1][0]) for r in CFGS}
  assert 64 in spbs and min(spbs) < 16                             # capped at 64 / by LDS
  assert all(T <= 100 for _, T in _tbwd_cases())
  for cases in (_bwd_cases(), _tbwd_cases()):
    rows = [CFGS[ci] for ci, _ in cases]
    assert any(r[1][0] > 0 for r in rows) and any(r[5] for r in rows) and {r[4] for r in rows} == {True, False}
    assert {r[3] for r in rows} == {'cone', 'cylinder'}


def _sum64(gA, gB):
  return gA.double() + (gB.double() if gB is not None else 0.0)


@pytest.mark.parametrize('case', _bwd_cases(), ids=lambda c: f'{_cfg(CFGS[c[0]])["id"]}-T{c[1]}')
def test_ipe_leaf_bwd(ops, case):
  """mnr_cast_rays_ipe_bwd with two gradient sources and with one."""
  cfg = _cfg(CFGS[case[0]])
  inp = _case_inputs(_bwd_cases(), case, _spb_bwd(cfg['K'], cfg['L']), 3000)
  M = inp['B'] * inp['n']
  gA, gB = _upstream(3100 + case[1], M, cfg, cfg['ld'], 1), _upstream(3200 + case[1], M, cfg, cfg['ld'], 1)
  items = []
  for name, b in (('two sources', gB), ('one source', None)):
    G = _sum64(gA, b)
    items.append((name, _kernel_bwd(ops, cfg, inp, gA, b), _ref_grad(cfg, inp, f64, G), _ref_grad(cfg, inp, f32, G), FLOOR_BWD))
  _hold_rays(f'ipe_leaf_bwd {cfg["id"]} B={inp["B"]} n={inp["n"]}', items)


def _init_for(seed, ref, B, n):
  """Non-zero g_t0 / g_t1 to accumulate onto, at the scale of the gradient; -> (init0, init1 fp32 [M], their sum per interval end)."""
  g = torch.Generator().manual_seed(seed)
  s = float(ref.abs().median().clamp(min=1e-30))
  i0, i1 = ((torch.randn(B * n, generator=g, dtype=f64) * s).float() for _ in range(2))
  return i0, i1, _fence(B, n, i0, i1)


@pytest.mark.parametrize('case', _tbwd_cases(), ids=lambda c: f'{_cfg(CFGS[c[0]])["id"]}-T{c[1]}')
def test_ipe_leaf_tangent_bwd(ops, case):
  """mnr_cast_rays_ipe_tangent_bwd with two gradient sources and with one, accumulating onto non-zero g_t0 / g_t1 (the
  reference adds the same numbers, the fp32 oracle adds them in fp32)."""
  cfg = _cfg(CFGS[case[0]])
  inp = _case_inputs(_tbwd_cases(), case, SPB_TBWD, 4000)
  B, n = inp['B'], inp['n']
  M = B * n
  gA, gB = _upstream(4100 + case[1], 3 * M, cfg, cfg['ld'], 2), _upstream(4200 + case[1], 3 * M, cfg, cfg['ld'], 2)
  items = []
  for name, b in ((('two sources', gB), ('one source', None)) if case != TBWD_K21 else (('two sources', gB),)):
    G = _sum64(gA, b)
    r64, r32 = _ref_grad(cfg, inp, f64, G, True), _ref_grad(cfg, inp, f32, G, True)
    i0, i1, init = _init_for(4300 + case[1], r64, B, n)
    got = _kernel_tbwd(ops, cfg, inp, gA, b, i0, i1)
    items.append((name, got, r64 + init, (r32 + init.float()).double(), FLOOR_BWD))
  _hold_rays(f'ipe_leaf_tangent_bwd {cfg["id"]} B={B} n={n}', items)


@pytest.mark.parametrize('shape,contract', SMALL_VARIANTS)
def test_ipe_leaf_small_scene_bwd(ops, shape, contract):
  """Both VJPs in the small scene ONE DEGREE AT A TIME (the upstream gradient is zero outside the degree): every degree
  0..15 under YARD_MAX at an amplitude of 0.5 or more."""
  cfg = _small_cfg(shape, contract)
  inp = _rays(31, 7, 5, 'small')
  B, n, M = 7, 5, 35
  r64 = _ref_rows(cfg, inp, f64)
  assert (_deg_max(r64, cfg) >= 0.5).all()
  for tangent in (False, True):
    items = []
    for l in range(16):
      gA = _upstream(5000 + l, (3 if tangent else 1) * M, cfg, cfg['ld'], 2 if tangent else 1, degree=l)
      G = gA.double()
      g64, g32 = _ref_grad(cfg, inp, f64, G, tangent), _ref_grad(cfg, inp, f32, G, tangent)
      if tangent:
        z = torch.zeros(M)
        got = _kernel_tbwd(ops, cfg, inp, gA, None, z, z)
      else:
        got = _kernel_bwd(ops, cfg, inp, gA, None)
      items.append((f'deg{l}', got, g64, g32, FLOOR_BWD))
    res = _hold_rays(f'ipe_leaf_small_scene_bwd {shape} contract={contract} {"tangent " if tangent else ""}VJP', items)
    assert all(y <= YARD_MAX for _, y in res.values()), res


# ----------------------------------------------------------------------------- caller-supplied Gaussians


def _gaussians(seed, M, small=False):
  """General covariances A A^T (not ray-shaped), exactly symmetric; means on both sides of |x| = 1 (small: the small scene's)."""
  g = torch.Generator().manual_seed(seed)
  if small:
    means = (torch.rand((M, 3), generator=g, dtype=f64) * 2 - 1) * 2.0 ** -5 + 2.0 ** -6
    sigma = torch.full((M, 1, 1), 1e-6, dtype=f64)
  else:
    means = (torch.rand((M, 3), generator=g, dtype=f64) * 2 - 1) * 1.1
    sigma = 10.0 ** (-4 + 2.5 * torch.rand((M, 1, 1), generator=g, dtype=f64))
  A = torch.randn((M, 3, 3), generator=g, dtype=f64) * sigma
  cov = A @ A.transpose(-1, -2)
  cov = 0.5 * (cov + cov.transpose(-1, -2))
  return means.float(), cov.float()


def _gs_cases():
  return _fwd_cases()


def _gs_refs(cfg, means, covs, dtype, tangent=False):
  m0, c0 = means.to(dtype), covs.to(dtype)
  if tangent:
    return _tangent_rows(cfg, m0, c0)
  m1, c1 = ocoord.track_linearize(ocoord.contract, m0, c0) if cfg['contract'] else (m0, c0)
  return _encode(cfg, m1, c1), m1, c1


def _run_gaussians(ops, label, cfg, means, covs):
  M = means.shape[0]
  kw = dict(warp_contract=cfg['contract'], min_deg=cfg['min_deg'], max_deg=cfg['max_deg'], ld_feat=cfg['ld'])
  (r64, m64, c64), (r32, m32, c32) = _gs_refs(cfg, means, covs, f64), _gs_refs(cfg, means, covs, f32)
  buf, out = _guarded(M, cfg['ld'], bf16)
  has32 = cfg['F'] % 4 == 0
  res = ops.ipe_from_gaussians(dev(means), dev(covs.reshape(M, 9)), dev(cfg['P']), out=out, want_f32=has32, want_gaussians=True, **kw)
  torch.cuda.synchronize()
  assert _guard_ok(buf), 'bf16 rows: guard row'
  rows32 = res[1] if has32 else None
  gm, gc = res[-2], res[-1]
  yard = None
  if has32:
    _, yard = _hold_rows(label + ' f32', cfg, rows32, r64, r32, FLOOR_FWD, _arg_max(cfg, m64))
  _check_bf16(label + ' bf16', cfg, out, rows32, r64, r32, _arg_max(cfg, m64))
  _hold_rays(label, [('means', gm, m64, m32, FLOOR_GAUSS), ('covs', gc, c64.reshape(M, 9), c32.reshape(M, 9), FLOOR_GAUSS)])
  return r64, yard


def _run_gaussians_tangent(ops, label, cfg, means, covs):
  M = means.shape[0]
  t64, t32 = _gs_refs(cfg, means, covs, f64, True), _gs_refs(cfg, means, covs, f32, True)
  buf, out = _guarded(3 * M, cfg['ld'], bf16)
  ops.ipe_from_gaussians_tangent(dev(means), dev(covs.reshape(M, 9)), dev(cfg['P']), warp_contract=cfg['contract'], min_deg=cfg['min_deg'],
                                 max_deg=cfg['max_deg'], ld_feat=cfg['ld'], out=out)
  torch.cuda.synchronize()
  assert _guard_ok(buf), 'tangent rows: guard row'
  return _check_bf16(label + ' tangent', cfg, out, None, t64, t32, _arg_max(cfg, _gs_refs(cfg, means, covs, f64)[1]), FLOOR_TAN, scale_floor=True)


@pytest.mark.parametrize('case', _gs_cases(), ids=lambda c: f'{_cfg(CFGS[c[0]])["id"]}-M{c[1]}')
def test_ipe_leaf_gaussians(ops, case):
  """mnr_ipe_from_gaussians (bf16 rows, want_f32, the post-warp Gaussians) on general covariances."""
  cfg = _cfg(CFGS[case[0]])
  means, covs = _gaussians(6000 + 100 * case[0] + case[1], case[1])
  if cfg['contract'] and case[1] >= 16:
    assert _both_sides(cfg, means.double())
  _run_gaussians(ops, f'ipe_leaf_gaussians {cfg["id"]} M={case[1]}', cfg, means, covs)


@pytest.mark.parametrize('case', _tan_cases(), ids=lambda c: f'{_cfg(CFGS[c[0]], 48)["id"]}-M{c[1]}')
def test_ipe_leaf_gaussians_tangent(ops, case):
  cfg = _cfg(CFGS[case[0]], 48)
  means, covs = _gaussians(7000 + 100 * case[0] + case[1], case[1])
  _run_gaussians_tangent(ops, f'ipe_leaf_gaussians {cfg["id"]} M={case[1]}', cfg, means, covs)


def test_ipe_leaf_small_scene_gaussians(ops):
  cfg = _small_cfg('cone', False)
  means, covs = _gaussians(32, 35, small=True)
  label = 'ipe_leaf_small_scene_gaussians'
  r64, yard = _run_gaussians(ops, label, cfg, means, covs)
  _assert_coverage(label, cfg, yard, r64)
  _, yard_t = _run_gaussians_tangent(ops, label, cfg, means, covs)
  _assert_coverage(label + ' tangent', cfg, yard_t, r64, scale=2.0 ** torch.arange(16).double())


# ----------------------------------------------------------------------------- edge inputs

EDGES = ['zero_width', 'all_coincide', 'origin_eps_clamp', 'radius_0', 't_6e5', 'negative_t', 'on_unit_sphere', 'tiny_direction',
         'radius_x300']


def _edge(name):
  """-> (configuration, inputs): B = 3, n = 4, octahedron, degrees [0, 16); the edge is planted in ray 0 (or in all rays)."""
  contract = name in ('origin_eps_clamp', 'on_unit_sphere', 'zero_width', 'radius_x300')
  cfg = _cfg(('octa1', (0, 16), 'up8', 'cone', contract, False))
  inp = _rays(8000 + EDGES.index(name), 3, 4, radius_scale=300.0 if name == 'radius_x300' else 1.0)
  t, o, d = inp['tdist'], inp['o'], inp['d']
  if name == 'zero_width':
    t[0, 2] = t[0, 1]
  elif name == 'all_coincide':
    t[0, :] = t[0, 2]
  elif name == 'origin_eps_clamp':                       # the mean AT the origin: |x|^2 is clamped to eps under the contraction
    o[0] = 0.0
    t[0, 0] = t[0, 1] = 0.0
  elif name == 'radius_0':
    inp['radii'][:] = 0.0
  elif name == 't_6e5':                                  # safe_sin's wrap at 100 pi is reached from degree 0 on (ray 0), 4 (ray 1), 8 (ray 2);
    far = torch.tensor([[6e5], [3e4], [2e3]], dtype=f64)  # narrow intervals and thin rays, so that the low degrees are not attenuated away
    inp['tdist'] = (far - 0.25 * torch.arange(4, -1, -1, dtype=f64)).float()
    inp['radii'][:] = 1e-9
  elif name == 'negative_t':
    inp['tdist'] = (t - 1.5).float()
  elif name == 'on_unit_sphere':
    o[0] = torch.tensor([1.0, 0.0, 0.0])
    d[0] = torch.tensor([0.0, 1.0, 0.0])
    t[0] = 1e-4 * (1 + torch.arange(5, dtype=f32))
  elif name == 'tiny_direction':
    d[0] = d[0] * 1e-6
  return cfg, inp


def test_ipe_leaf_edge_table_covers_every_value():
  assert len(EDGES) == 9 and len(set(EDGES)) == 9
  for name in EDGES:
    cfg, inp = _edge(name)
    t = inp['tdist']
    assert torch.isfinite(t).all() and (t[:, 1:] >= t[:, :-1]).all()
  assert _edge('t_6e5')[1]['tdist'].max() > 5e5 and _edge('negative_t')[1]['tdist'].min() < 0
  assert _edge('tiny_direction')[1]['d'][0].norm() < 2e-6 and _edge('radius_x300')[1]['radii'].min() > 0.05


@pytest.mark.parametrize('name', EDGES)
def test_ipe_leaf_edge_inputs(ops, name):
  """Forward (bf16 and fp32 rows, under the usual bounds) and mnr_cast_rays_ipe_bwd: finite wherever the fp64 reference is."""
  cfg, inp = _edge(name)
  M = 12
  r64, r32 = _ref_rows(cfg, inp, f64), _ref_rows(cfg, inp, f32)
  assert torch.isfinite(r64).all()
  if name == 't_6e5':
    assert _deg_max(r64, cfg)[0] >= 0.5 and _ray_arg(cfg, inp)[0] > 100 * math.pi     # the wrap is reached on features that are alive
  rows32 = _kernel_fwd(ops, cfg, inp, f32_rows=True)
  rows, means, covs = _kernel_fwd(ops, cfg, inp)
  for x in (rows32, rows.float(), means, covs):
    assert torch.isfinite(x.cpu()).all(), f'{name}: a forward output is not finite'
  _hold_rows(f'ipe_leaf_edge {name} f32', cfg, rows32, r64, r32, FLOOR_FWD, _ray_arg(cfg, inp))
  _check_bf16(f'ipe_leaf_edge {name} bf16', cfg, rows, rows32, r64, r32, _ray_arg(cfg, inp))
  gA = _upstream(8100, M, cfg, cfg['ld'], 1)
  g64 = _ref_grad(cfg, inp, f64, gA.double())
  got = _kernel_bwd(ops, cfg, inp, gA, None)
  fin = torch.isfinite(g64)
  assert torch.isfinite(got[fin]).all(), f'{name}: a gradient is not finite where the fp64 reference is'
  if fin.all():
    g32 = _ref_grad(cfg, inp, f32, gA.double())
    if torch.isfinite(g32).all():
      fig, yard = _ray_figure(got, g64), _ray_figure(g32, g64)
      print(f'ipe_leaf_edge {name} bwd: error {fig:.3e}, fp32 oracle {yard:.3e}, error / bound {_ratio(fig, max(MARGIN * yard, FLOOR_BWD)):.3f} (printed, not asserted)')


# ----------------------------------------------------------------------------- the launchers' refusals


def _tangent_call(ops, cfg, inp, out):
  return ops.cast_rays_ipe_tangent(*_dev_rays(inp), dev(cfg['P']), ld_feat=cfg['ld'], out=out, **_kw(cfg))


LDS_ROWS = {8: ('unit1', (0, 4)), 24: ('octa1', (0, 4)), 40: ('ico1', (0, 3)), 48: ('octa1', (0, 8))}


@pytest.mark.parametrize('ld', sorted(LDS_ROWS))
def test_ipe_leaf_lds_refusal(ops, ld):
  """Three tangent rows per sample of ld_feat <= 40 need more than 64 KiB of LDS per block: both launchers refuse them before
  anything is launched, with the same message; ld_feat = 48 fits, runs and matches fp64."""
  basis, degs = LDS_ROWS[ld]
  cfg = _cfg((basis, degs, 'up8', 'cone', False, False))
  assert cfg['ld'] == ld and (_lds_fwd(ld, cfg['K'], True) > 65536) == (ld <= 40)
  inp = _rays(9000 + ld, 3, 5)
  M = 15
  buf, out = _guarded(3 * M, ld, bf16)
  if ld <= 40:
    msgs = []
    with pytest.raises(ValueError, match='bytes of LDS per block') as e:
      _tangent_call(ops, cfg, inp, out)
    msgs.append(str(e.value))
    means, covs = _gaussians(9001, M)
    with pytest.raises(ValueError, match='bytes of LDS per block') as e:
      ops.ipe_from_gaussians_tangent(dev(means), dev(covs.reshape(M, 9)), dev(cfg['P']), warp_contract=False, min_deg=degs[0], max_deg=degs[1],
                                     ld_feat=ld, out=out)
    msgs.append(str(e.value))
    torch.cuda.synchronize()
    assert (buf.float().cpu() == SENT).all(), 'a refused call wrote to its output'
    assert msgs[0].split(':', 1)[1] == msgs[1].split(':', 1)[1] and str(_lds_fwd(ld, cfg['K'], True)) in msgs[0], msgs
  else:
    _tangent_call(ops, cfg, inp, out)
    torch.cuda.synchronize()
    assert _guard_ok(buf)
    _check_bf16(f'ipe_leaf_lds_refusal ld={ld}', cfg, out, None, _ref_rows(cfg, inp, f64, True), _ref_rows(cfg, inp, f32, True), _ray_arg(cfg, inp), FLOOR_TAN,
                scale_floor=True)


def test_ipe_leaf_refusals(ops):
  """What the launchers refuse before any launch: each is a ValueError and leaves the outputs alone."""
  inp = _rays(9100, 2, 3)
  M = 6
  a = _dev_rays(inp)
  octa = dev(_basis('octa1'))

  def bf(ld):
    return torch.full((M, ld), SENT, dtype=bf16).cuda()

  def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t.float().cpu() == SENT).all()) for t in ts)

  kw = dict(ray_shape='cone', warp_contract=False)
  # K > 128
  big = dev(torch.nn.functional.normalize(torch.randn((129, 3), generator=torch.Generator().manual_seed(1)), dim=-1))
  out = bf(264)
  with pytest.raises(ValueError, match='basis_k=129'):
    ops.cast_rays_ipe(*a, big, min_deg=0, max_deg=1, ld_feat=264, out=out, **kw)
  g0, g1 = torch.full((M,), SENT).cuda(), torch.full((M,), SENT).cuda()
  with pytest.raises(ValueError, match='basis_k=129'):
    ops.cast_rays_ipe_bwd(*a, big, bf(264), None, min_deg=0, max_deg=1, g_t0=g0, g_t1=g1, **kw)
  with pytest.raises(ValueError, match='basis_k=129'):
    ops.cast_rays_ipe_tangent_bwd(*a, big, torch.zeros((3 * M, 264), dtype=bf16).cuda(), None, g0, g1, min_deg=0, max_deg=1, **kw)
  assert untouched(out, g0, g1)
  # L > 32
  out = bf(200)
  with pytest.raises(ValueError, match='degrees=33'):
    ops.cast_rays_ipe(*a, octa, min_deg=0, max_deg=33, ld_feat=200, out=out, **kw)
  with pytest.raises(ValueError, match='degrees=33'):
    ops.cast_rays_ipe_bwd(*a, octa, bf(200), None, min_deg=0, max_deg=33, g_t0=g0, g_t1=g1, **kw)
  assert untouched(out, g0, g1)
  # ld_feat < 2KL, ld_feat % 8 != 0
  for ld in (16, 28):
    out = bf(ld)
    with pytest.raises(ValueError, match='must be >= 24 and a multiple of 8'):
      ops.cast_rays_ipe(*a, octa, min_deg=0, max_deg=4, ld_feat=ld, out=out, **kw)
    with pytest.raises(ValueError, match='must be >= 24 and a multiple of 8'):
      ops.cast_rays_ipe_bwd(*a, octa, bf(ld), None, min_deg=0, max_deg=4, g_t0=g0, g_t1=g1, **kw)
    means, covs = _gaussians(9101, M)
    with pytest.raises(ValueError, match='must be >= 24 and a multiple of 8'):
      ops.ipe_from_gaussians(dev(means), dev(covs.reshape(M, 9)), octa, warp_contract=False, min_deg=0, max_deg=4, ld_feat=ld, out=out)
    assert untouched(out, g0, g1)
  out = torch.full((3 * M, 16), SENT, dtype=bf16).cuda()
  with pytest.raises(ValueError, match='must be >= 24'):
    ops.cast_rays_ipe_tangent_bwd(*a, octa, out, None, g0, g1, min_deg=0, max_deg=4, **kw)
  assert untouched(g0, g1)
  # fp32 rows with 2KL % 4 != 0 (through the C ABI: the front end allocates its own output)
  o32 = torch.full((M, 6), SENT).cuda()
  c = ops._ipe_cfg('cone', False, False, octa, 1, 2)
  with pytest.raises(ValueError, match='feature count must be a multiple of 4'):
    ops.L.check(ops.lib().mnr_cast_rays_ipe_f32(C.byref(c), 2, 3, *[ops._ptr(x) for x in a], ops._ptr(octa), ops._ptr(o32), ops._stream()))
  out = bf(8)
  means, covs = _gaussians(9102, M)
  with pytest.raises(ValueError, match='feature count must be a multiple of 4'):
    ops.ipe_from_gaussians(dev(means), dev(covs.reshape(M, 9)), octa, warp_contract=False, min_deg=1, max_deg=2, ld_feat=8, out=out, want_f32=True)
  assert untouched(o32, out)                            # (the bf16 pass in front of the refused fp32 pass included)
  # a bad ray_shape: the front end's own refusal, and the launchers' behind it
  out = bf(24)
  with pytest.raises(ValueError, match='ray_shape'):
    ops.cast_rays_ipe(*a, octa, ray_shape='sphere', warp_contract=False, min_deg=0, max_deg=4, ld_feat=24, out=out)
  c = ops.L.IpeCfg(2, 0, 0, 3, 0, 4)
  p = [ops._ptr(x) for x in a] + [ops._ptr(octa)]
  lib = ops.lib()
  g_in = torch.zeros((3 * M, 24), dtype=bf16).cuda()
  for call in (lambda: lib.mnr_cast_rays_ipe(C.byref(c), 2, 3, *p, ops._ptr(out), 24, None, None, ops._stream()),
               lambda: lib.mnr_cast_rays_ipe_tangent(C.byref(c), 2, 3, *p, ops._ptr(out), 24, ops._stream()),
               lambda: lib.mnr_cast_rays_ipe_bwd(C.byref(c), 2, 3, *p, ops._ptr(g_in), None, 24, ops._ptr(g0), ops._ptr(g1), ops._stream()),
               lambda: lib.mnr_cast_rays_ipe_tangent_bwd(C.byref(c), 2, 3, *p, ops._ptr(g_in), None, 24, ops._ptr(g0), ops._ptr(g1), ops._stream())):
    with pytest.raises(ValueError, match='ray_shape'):
      ops.L.check(call())
  assert untouched(out, g0, g1)


# ----------------------------------------------------------------------------- mnr_viewdir_enc_fill


def _view_layout(kind, nenc):
  """-> (col0, col_end, ld, element offset of the view, vectorised?): the launcher's condition restated."""
  span = (nenc + 7) // 8 * 8 + 8
  if kind == 'aligned':
    lay = (8, 8 + span, 8 + span + 8, 0)
  elif kind == 'col0_3':
    lay = (3, 3 + span, 8 + span + 8, 0)
  elif kind == 'ld_odd':
    lay = (8, 8 + span, max(83, 8 + span + 3) | 1, 0)
  else:                                                   # 'offset1': the aligned layout in a view that starts one element in
    lay = (8, 8 + span, 8 + span + 8, 1)
  col0, col_end, ld, off = lay
  vec = col0 % 8 == 0 and (col_end - col0) % 8 == 0 and ld % 8 == 0 and off % 8 == 0
  return lay + (vec,)


VIEW_LAYOUTS = ('aligned', 'col0_3', 'ld_odd', 'offset1')


def test_ipe_leaf_viewdir_table_covers_every_value():
  lays = {k: _view_layout(k, 27) for k in VIEW_LAYOUTS}
  assert [lays[k][4] for k in VIEW_LAYOUTS] == [True, False, False, False]
  assert lays['col0_3'][0] == 3 and lays['ld_odd'][2] == 83 and lays['offset1'][3] == 1
  assert lays['aligned'][:3] == lays['offset1'][:3]                                  # a layout both kernels accept


@pytest.mark.parametrize('B', [1, 37])
@pytest.mark.parametrize('n', [1, 7, 8, 13])
@pytest.mark.parametrize('deg', [0, 1, 4, 16])
def test_ipe_leaf_viewdir_enc_fill(ops, deg, n, B):
  """Both kernels against coord.pos_enc(..., append_identity=True) in fp64 at half a bf16 ulp plus the per-degree bound; zeros up
  to col_end; everything outside [col0, col_end) and behind the matrix untouched; the two kernels bit-equal."""
  g = torch.Generator().manual_seed(10000 + deg)
  v = torch.randn((B, 3), generator=g, dtype=f64)
  v = (v / v.norm(dim=-1, keepdim=True)).float()
  nenc = 3 + 6 * deg
  r64, r32 = ocoord.pos_enc(v.double(), 0, deg, True), ocoord.pos_enc(v, 0, deg, True).double()
  # the bound per column: the identity exactly; degree l from the fp32 oracle's own error at that degree
  bound = torch.zeros(nenc, dtype=f64)
  worst_yard = 0.0
  for l in range(deg):
    cols = [3 + h * 3 * deg + 3 * l + i for h in (0, 1) for i in range(3)]
    yard = (r32[:, cols] - r64[:, cols]).abs().max().item()
    worst_yard = max(worst_yard, yard)
    bound[cols] = max(MARGIN * yard, FLOOR_VIEW)
  rows = B * n
  filled = {}
  worst = 0.0
  for kind in VIEW_LAYOUTS:
    col0, col_end, ld, off, vec = _view_layout(kind, nenc)
    buf = torch.full((off + (rows + 1) * ld,), SENT, dtype=bf16).cuda()
    dst = buf[off:off + rows * ld].view(rows, ld)
    assert (dst.data_ptr() % 16 == 0) == (off == 0)
    ops.viewdir_enc_fill(dev(v), n, deg, dst, col0, col_end)
    torch.cuda.synchronize()
    flat = buf.float().cpu()
    assert (flat[:off] == SENT).all() and (flat[off + rows * ld:] == SENT).all(), f'{kind}: wrote outside the matrix'
    out = flat[off:off + rows * ld].reshape(B, n, ld).double()
    assert (out[..., :col0] == SENT).all() and (out[..., col_end:] == SENT).all(), f'{kind}: wrote outside [col0, col_end)'
    assert (out[..., col0 + nenc:col_end] == 0).all(), f'{kind}: no zeros up to col_end'
    enc = out[..., col0:col0 + nenc]
    want = r64[:, None, :].expand(B, n, nenc)
    ratio = ((enc - want).abs() / (_half_ulp_bf16(want, bound) + bound).clamp(min=1e-300)).max().item()
    assert (enc[..., :3] == v[:, None, :].to(bf16).double()).all(), f'{kind}: the identity columns are not the rounded directions'
    worst = max(worst, ratio)
    assert ratio <= 1.0, f'{kind}: error / bound {ratio:.3f}'
    filled[kind] = buf[off:off + rows * ld].view(rows, ld)[:, col0:col_end].cpu()
  print(f'ipe_leaf_viewdir deg={deg} n={n} B={B}: worst error / bound {worst:.3f} (fp32 oracle {worst_yard:.2e})')
  assert torch.equal(filled['aligned'].view(torch.int16), filled['offset1'].view(torch.int16)), 'the two kernels differ on one layout'


# ----------------------------------------------------------------------------- mnr_glo_fill, mnr_glo_bwd


@pytest.mark.parametrize('G', [1, 4, 7])
def test_ipe_leaf_glo(ops, G):
  """Indices below 0 and at or above num_embeddings are clamped; cam_idx = None fills zeros; several rays share an index; the
  VJP with and without g_b, accumulating onto a non-zero table gradient."""
  g = torch.Generator().manual_seed(11000 + G)
  B, n, E, ld, col0 = 11, 3, 5, 19, 6
  table = torch.randn((E, G), generator=g)
  cam = torch.tensor([-3, -1, 0, 0, 2, 2, 2, 4, 5, 9, 1], dtype=torch.int32)
  idx = cam.long().clamp(0, E - 1)
  buf, dst = _guarded(B * n, ld, bf16)
  ops.glo_fill(dev(table), dev(cam), B, n, dst, col0)
  torch.cuda.synchronize()
  got = buf.cpu()
  assert torch.equal(got[:B * n, col0:col0 + G], table[idx].repeat_interleave(n, 0).to(bf16))
  keep = torch.ones(ld, dtype=torch.bool)
  keep[col0:col0 + G] = False
  assert (got[:B * n][:, keep].float() == SENT).all() and _guard_ok(buf)
  ops.glo_fill(dev(table), None, B, n, dst, col0)
  torch.cuda.synchronize()
  got = buf.cpu()
  assert not got[:B * n, col0:col0 + G].float().any() and (got[:B * n][:, keep].float() == SENT).all() and _guard_ok(buf)
  ga, gb = torch.randn((B * n, G), generator=g), torch.randn((B * n, G), generator=g)
  init = torch.randn((E + 1, G), generator=g)
  for b in (gb, None):
    grad = init.clone().cuda()
    ops.glo_bwd(dev(ga), dev(b), dev(cam), B, n, grad.view(-1)[:E * G], E, G)
    torch.cuda.synchronize()
    assert torch.equal(grad[E].cpu(), init[E]), 'guard row of the table gradient'
    terms = ga.double() + (b.double() if b is not None else 0.0)
    per_ray = terms.view(B, n, G).sum(1)
    r64 = init[:E].double().index_add(0, idx, per_ray)
    t32 = ga if b is None else ga + b
    r32 = init[:E].clone().index_add(0, idx, t32.view(B, n, G).sum(1)).double()
    count = torch.zeros(E, dtype=f64).index_add(0, idx, torch.full((B,), float(n * (2 if b is not None else 1) + 1), dtype=f64))
    mag = init[:E].double().abs().index_add(0, idx, (ga.double().abs() + (b.double().abs() if b is not None else 0.0)).view(B, n, G).sum(1))
    yard = (r32 - r64).abs()
    bound = torch.maximum(MARGIN * yard, count[:, None] * U * mag)
    ratio = ((grad[:E].cpu().double() - r64).abs() / bound.clamp(min=1e-300)).max().item()
    print(f'ipe_leaf_glo G={G} g_b={"yes" if b is not None else "no"}: worst error / bound {ratio:.3f}')
    assert ratio <= 1.0
    untouched = torch.ones(E, dtype=torch.bool)
    untouched[idx] = False
    assert torch.equal(grad[:E].cpu()[untouched], init[:E][untouched])
