"""Torch-tensor front ends for the C ABI (include/mnerf.h).

torch is plumbing here: it owns device memory and the stream; all arithmetic on
the hot path happens inside libmnerf_hip.so.  Every function validates device,
dtype and contiguity and then passes raw device pointers.
"""

import ctypes as C
import math
import os

import numpy as np
import torch

from multinerf_amd import _lib as L

bf16 = torch.bfloat16
f32 = torch.float32


def _ptr(t):
  return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_device(t):
  return t.is_cuda


def act_dtype():
  """Storage type of the Dense layers' activation / gradient / packed-weight matrices: bf16, or fp32 inside
  `_lib.dense_f32()` (the fp32-Dense debug build, Model(dense_precision='fp32'))."""
  return f32 if L.f32_active() else bf16


def _chk(t, dtype, name, allow_none=False):
  if dtype is bf16 and L.f32_active():
    dtype = f32
  if t is None:
    if allow_none:
      return
    raise ValueError(f'{name} is None')
  if not _on_device(t):
    raise ValueError(f'{name} must be a device tensor (the HIP path has no CPU fallback)')
  if t.dtype != dtype:
    raise ValueError(f'{name} must be {dtype}, is {t.dtype}')
  if not t.is_contiguous():
    raise ValueError(f'{name} must be contiguous')


def lib():
  """The loaded C-ABI library (include/mnerf.h).  No process-global switches are applied: the development hooks of
  include/mnerf_debug.h are reached through multinerf_amd._lib.debug() by tests and tools only."""
  return L.load()


class _GemmProfile:
  """Optional HIP-event timing of kernel launches on the launch stream (bench.py roofline): GEMMs under the tag
  'gemm', the bandwidth-bound kernels under their own tags together with their algorithmic HBM bytes."""

  def __init__(self):
    self.on = False
    self.events = []

  def enable(self):
    self.on, self.events = True, []
    self.base = torch.cuda.Event(enable_timing=True)     # time origin for the busy-time union across streams
    self.base.record(torch.cuda.current_stream())

  def disable(self):
    self.on = False

  def start(self):
    if not self.on:
      return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream())
    return e0

  def stop(self, e0, tag='gemm', nbytes=0):
    if e0 is None:
      return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record(torch.cuda.current_stream())
    self.events.append((e0, e1, tag, nbytes))

  def collect(self):
    """-> (total GEMM ms, GEMM launches); call after a synchronize.  Other tags: collect_by_tag() first."""
    by = self.collect_by_tag()
    g = by.get('gemm', dict(ms=0.0, launches=0))
    return g['ms'], g['launches']

  def collect_by_tag(self):
    """-> {tag: {'ms', 'launches', 'bytes'}}; empties the event list."""
    out, spans = {}, {}
    for a, b, tag, nbytes in self.events:
      d = out.setdefault(tag, dict(ms=0.0, launches=0, bytes=0))
      d['ms'] += a.elapsed_time(b)
      d['launches'] += 1
      d['bytes'] += nbytes
      spans.setdefault(tag, []).append((self.base.elapsed_time(a), self.base.elapsed_time(b)))
    # 'busy_ms': length of the UNION of the tag's launch intervals (= 'ms' when the launches are serial on one stream;
    # less when two streams run kernels of the tag side by side, multinerf_amd/streams.py)
    for tag, iv in spans.items():
      iv.sort()
      busy, end = 0.0, None
      for a0, b0 in iv:
        if end is None or a0 > end:
          busy += b0 - a0
          end = b0
        elif b0 > end:
          busy += b0 - end
          end = b0
      out[tag]['busy_ms'] = busy
    self.events = []
    return out


PROFILE = _GemmProfile()


# ----------------------------------------------------------------------------- sampling


def resample_level(sdist_prev, w_prev, u_base, jitter, near, far, *, n_samples, use_dilation,
                   dilation, domain, anneal, resample_padding, single_jitter, max_jitter,
                   raydist_fn, want_idx=False):
  for t, nm in ((sdist_prev, 'sdist_prev'), (w_prev, 'w_prev'), (u_base, 'u_base'),
                (near, 'near'), (far, 'far')):
    _chk(t, f32, nm)
  _chk(jitter, f32, 'jitter', allow_none=True)
  B, n_prev = w_prev.shape
  assert sdist_prev.shape == (B, n_prev + 1) and u_base.numel() == n_samples
  assert near.numel() == B and far.numel() == B
  if jitter is not None:
    assert jitter.numel() == (B if single_jitter else B * n_samples)
  cfg = L.ResampleCfg(n_prev, n_samples, int(use_dilation), float(dilation), float(domain[0]),
                      float(domain[1]), float(anneal), float(resample_padding), int(single_jitter),
                      float(max_jitter), L.RAYDIST[raydist_fn])
  dev = w_prev.device
  sdist = torch.empty((B, n_samples + 1), dtype=f32, device=dev)
  tdist = torch.empty((B, n_samples + 1), dtype=f32, device=dev)
  idx = torch.empty((B, n_samples), dtype=torch.int32, device=dev) if want_idx else None
  _e = PROFILE.start()
  L.check(lib().mnr_resample_level(C.byref(cfg), B, _ptr(sdist_prev), _ptr(w_prev), _ptr(u_base),
                                   _ptr(jitter), _ptr(near), _ptr(far), _ptr(sdist), _ptr(tdist),
                                   _ptr(idx), _stream()))
  PROFILE.stop(_e, 'resample', 4 * (sdist_prev.numel() + w_prev.numel() + 2 * sdist_prev.shape[0] * (n_samples + 1)))
  return (sdist, tdist, idx) if want_idx else (sdist, tdist)


def resample_level_bwd(sdist_prev, w_prev, u_base, jitter, g_sdist, *, n_samples, use_dilation, dilation, domain, anneal,
                       resample_padding, single_jitter, max_jitter, raydist_fn, g_sdist_prev=None, g_w_prev=None):
  """VJP of `resample_level` w.r.t. (sdist_prev, w_prev) given g_sdist = d loss / d sdist (Model.stop_level_grad = False)."""
  for t, nm in ((sdist_prev, 'sdist_prev'), (w_prev, 'w_prev'), (u_base, 'u_base'), (g_sdist, 'g_sdist')):
    _chk(t, f32, nm)
  _chk(jitter, f32, 'jitter', allow_none=True)
  B, n_prev = w_prev.shape
  assert sdist_prev.shape == (B, n_prev + 1) and u_base.numel() == n_samples and g_sdist.shape == (B, n_samples + 1)
  if jitter is not None:
    assert jitter.numel() == (B if single_jitter else B * n_samples)
  cfg = L.ResampleCfg(n_prev, n_samples, int(use_dilation), float(dilation), float(domain[0]),
                      float(domain[1]), float(anneal), float(resample_padding), int(single_jitter),
                      float(max_jitter), L.RAYDIST[raydist_fn])
  dev = w_prev.device
  if g_sdist_prev is None:
    g_sdist_prev = torch.empty((B, n_prev + 1), dtype=f32, device=dev)
  if g_w_prev is None:
    g_w_prev = torch.empty((B, n_prev), dtype=f32, device=dev)
  _chk(g_sdist_prev, f32, 'g_sdist_prev')
  _chk(g_w_prev, f32, 'g_w_prev')
  assert g_sdist_prev.shape == (B, n_prev + 1) and g_w_prev.shape == (B, n_prev)
  L.check(lib().mnr_resample_level_bwd(C.byref(cfg), B, _ptr(sdist_prev), _ptr(w_prev), _ptr(u_base), _ptr(jitter),
                                       _ptr(g_sdist), _ptr(g_sdist_prev), _ptr(g_w_prev), _stream()))
  return g_sdist_prev, g_w_prev


def sorted_interp(u, cw, t):
  for x, nm in ((u, 'u'), (cw, 'cw'), (t, 't')):
    _chk(x, f32, nm)
  B, nc = cw.shape
  nu = u.shape[1]
  out = torch.empty_like(u)
  idx = torch.empty(u.shape, dtype=torch.int32, device=u.device)
  L.check(lib().mnr_sorted_interp(B, nc, nu, _ptr(u), _ptr(cw), _ptr(t), _ptr(out), _ptr(idx), _stream()))
  return out, idx


def max_dilate_weights(t, w, dilation, domain):
  _chk(t, f32, 't')
  _chk(w, f32, 'w')
  B, n = w.shape
  t_out = torch.empty((B, 3 * n + 1), dtype=f32, device=w.device)
  w_out = torch.empty((B, 3 * n), dtype=f32, device=w.device)
  scratch = torch.empty((B, n), dtype=f32, device=w.device)
  L.check(lib().mnr_max_dilate_weights(B, n, _ptr(t), _ptr(w), float(dilation), float(domain[0]),
                                       float(domain[1]), _ptr(t_out), _ptr(w_out), _ptr(scratch), _stream()))
  return t_out, w_out


# ----------------------------------------------------------------------------- features


def _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg):
  if ray_shape not in ('cone', 'cylinder'):
    raise ValueError('ray_shape must be \'cone\' or \'cylinder\'')   # render.py:124
  return L.IpeCfg(0 if ray_shape == 'cone' else 1, int(bool(warp_contract)), int(bool(disable_integration)),
                  basis.shape[0], int(min_deg), int(max_deg))


def cast_rays_ipe(tdist, origins, directions, radii, basis, *, ray_shape, warp_contract, min_deg,
                  max_deg, ld_feat, disable_integration=False, out=None, want_gaussians=False):
  """-> bf16 features [B*n, ld_feat] (+ optional post-warp means [B*n,3], covs [B*n,9])."""
  for x, nm in ((tdist, 'tdist'), (origins, 'origins'), (directions, 'directions'), (radii, 'radii'),
                (basis, 'basis')):
    _chk(x, f32, nm)
  B, n1 = tdist.shape
  n = n1 - 1
  cfg = _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg)
  dev = tdist.device
  if out is None:
    out = torch.empty((B * n, ld_feat), dtype=act_dtype(), device=dev)
  _chk(out, bf16, 'out')
  assert out.shape == (B * n, ld_feat)
  means = covs = None
  if want_gaussians:
    means = torch.empty((B * n, 3), dtype=f32, device=dev)
    covs = torch.empty((B * n, 9), dtype=f32, device=dev)
  _e = PROFILE.start()
  L.check(lib().mnr_cast_rays_ipe(C.byref(cfg), B, n, _ptr(tdist), _ptr(origins), _ptr(directions),
                                  _ptr(radii), _ptr(basis), _ptr(out), ld_feat, _ptr(means), _ptr(covs),
                                  _stream()))
  PROFILE.stop(_e, 'ipe', 4 * tdist.numel() + 2 * out.numel())
  return (out, means, covs) if want_gaussians else out


def cast_rays_ipe_f32(tdist, origins, directions, radii, basis, *, ray_shape, warp_contract, min_deg,
                      max_deg, disable_integration=False):
  for x, nm in ((tdist, 'tdist'), (origins, 'origins'), (directions, 'directions'), (radii, 'radii'),
                (basis, 'basis')):
    _chk(x, f32, nm)
  B, n1 = tdist.shape
  n = n1 - 1
  cfg = _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg)
  nfeat = 2 * basis.shape[0] * (max_deg - min_deg)
  out = torch.empty((B * n, nfeat), dtype=f32, device=tdist.device)
  L.check(lib().mnr_cast_rays_ipe_f32(C.byref(cfg), B, n, _ptr(tdist), _ptr(origins), _ptr(directions),
                                      _ptr(radii), _ptr(basis), _ptr(out), _stream()))
  return out


def cast_rays_ipe_tangent(tdist, origins, directions, radii, basis, *, ray_shape, min_deg, max_deg, ld_feat,
                          out=None, warp_contract=False, disable_integration=False):
  """-> bf16 [3*B*n, ld_feat]: rows c*B*n + s = d(features of sample s)/d(mean_c), mean = the pre-warp mean."""
  for x, nm in ((tdist, 'tdist'), (origins, 'origins'), (directions, 'directions'), (radii, 'radii'),
                (basis, 'basis')):
    _chk(x, f32, nm)
  B, n1 = tdist.shape
  n = n1 - 1
  cfg = _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg)
  if out is None:
    out = torch.empty((3 * B * n, ld_feat), dtype=act_dtype(), device=tdist.device)
  _chk(out, bf16, 'out')
  L.check(lib().mnr_cast_rays_ipe_tangent(C.byref(cfg), B, n, _ptr(tdist), _ptr(origins), _ptr(directions),
                                          _ptr(radii), _ptr(basis), _ptr(out), ld_feat, _stream()))
  return out


def _chk_gaussians(means, covs, basis):
  for x, nm in ((means, 'means'), (covs, 'covs'), (basis, 'basis')):
    _chk(x, f32, nm)
  if means.dim() != 2 or means.shape[1] != 3 or means.shape[0] == 0:
    raise ValueError(f'means must be [M, 3], is {tuple(means.shape)}')
  M = means.shape[0]
  if covs.numel() != M * 9 or covs.shape[0] != M:
    raise ValueError(f'covs must be [M, 9] or [M, 3, 3] (full covariances), is {tuple(covs.shape)}')
  return M


def ipe_from_gaussians(means, covs, basis, *, warp_contract, min_deg, max_deg, ld_feat, out=None, want_f32=False,
                       want_gaussians=False):
  """Caller-supplied Gaussians (means [M,3], covs [M,9] / [M,3,3], BEFORE the warp) -> bf16 features [M, ld_feat] as
  `cast_rays_ipe` writes them (+ optional fp32 features [M, 2KL], + optional post-warp means [M,3], covs [M,9])."""
  M = _chk_gaussians(means, covs, basis)
  cfg = _ipe_cfg('cone', warp_contract, False, basis, min_deg, max_deg)         # (ray_shape / disable_integration: not read)
  dev = means.device
  if out is None:
    out = torch.empty((M, ld_feat), dtype=act_dtype(), device=dev)
  _chk(out, bf16, 'out')
  assert out.shape == (M, ld_feat)
  feat32 = gm = gc = None
  if want_f32:
    feat32 = torch.empty((M, 2 * basis.shape[0] * (max_deg - min_deg)), dtype=f32, device=dev)
  if want_gaussians:
    gm = torch.empty((M, 3), dtype=f32, device=dev)
    gc = torch.empty((M, 9), dtype=f32, device=dev)
  _e = PROFILE.start()
  L.check(lib().mnr_ipe_from_gaussians(C.byref(cfg), M, _ptr(means), _ptr(covs), _ptr(basis), _ptr(out), ld_feat, _ptr(feat32),
                                       _ptr(gm), _ptr(gc), _stream()))
  PROFILE.stop(_e, 'ipe', 48 * M + 2 * out.numel())
  if not (want_f32 or want_gaussians):
    return out
  return (out,) + ((feat32,) if want_f32 else ()) + ((gm, gc) if want_gaussians else ())


def ipe_from_gaussians_tangent(means, covs, basis, *, warp_contract, min_deg, max_deg, ld_feat, out=None):
  """-> bf16 [3*M, ld_feat]: rows c*M + s = d(features of sample s)/d(mean_c), the covariance held fixed (as
  `cast_rays_ipe_tangent`, for caller-supplied Gaussians)."""
  M = _chk_gaussians(means, covs, basis)
  cfg = _ipe_cfg('cone', warp_contract, False, basis, min_deg, max_deg)
  if out is None:
    out = torch.empty((3 * M, ld_feat), dtype=act_dtype(), device=means.device)
  _chk(out, bf16, 'out')
  assert out.shape == (3 * M, ld_feat)
  L.check(lib().mnr_ipe_from_gaussians_tangent(C.byref(cfg), M, _ptr(means), _ptr(covs), _ptr(basis), _ptr(out), ld_feat,
                                               _stream()))
  return out


def cast_rays_ipe_bwd(tdist, origins, directions, radii, basis, g_feat_a, g_feat_b=None, *, ray_shape, warp_contract, min_deg,
                      max_deg, disable_integration=False, g_t0=None, g_t1=None):
  """VJP of `cast_rays_ipe` w.r.t. the interval ends: g_feat_a (+ g_feat_b) bf16 [B*n, ld] -> (g_t0, g_t1) fp32 [B*n]."""
  for x, nm in ((tdist, 'tdist'), (origins, 'origins'), (directions, 'directions'), (radii, 'radii'), (basis, 'basis')):
    _chk(x, f32, nm)
  _chk(g_feat_a, bf16, 'g_feat_a')
  _chk(g_feat_b, bf16, 'g_feat_b', allow_none=True)
  B, n1 = tdist.shape
  n = n1 - 1
  ld = g_feat_a.stride(0)
  assert g_feat_a.shape[0] == B * n and (g_feat_b is None or (g_feat_b.shape[0] == B * n and g_feat_b.stride(0) == ld))
  cfg = _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg)
  dev = tdist.device
  if g_t0 is None:
    g_t0 = torch.empty((B * n,), dtype=f32, device=dev)
  if g_t1 is None:
    g_t1 = torch.empty((B * n,), dtype=f32, device=dev)
  _chk(g_t0, f32, 'g_t0')
  _chk(g_t1, f32, 'g_t1')
  assert g_t0.numel() == B * n and g_t1.numel() == B * n
  L.check(lib().mnr_cast_rays_ipe_bwd(C.byref(cfg), B, n, _ptr(tdist), _ptr(origins), _ptr(directions), _ptr(radii), _ptr(basis),
                                      _ptr(g_feat_a), _ptr(g_feat_b), ld, _ptr(g_t0), _ptr(g_t1), _stream()))
  return g_t0, g_t1


def cast_rays_ipe_tangent_bwd(tdist, origins, directions, radii, basis, g_T_a, g_T_b, g_t0, g_t1, *, ray_shape, warp_contract, min_deg,
                              max_deg, disable_integration=False):
  """VJP of `cast_rays_ipe_tangent` w.r.t. the interval ends: g_T_a (+ g_T_b) bf16 [3*B*n, ld] -> g_t0, g_t1 fp32 [B*n] += ..."""
  for x, nm in ((tdist, 'tdist'), (origins, 'origins'), (directions, 'directions'), (radii, 'radii'), (basis, 'basis'),
                (g_t0, 'g_t0'), (g_t1, 'g_t1')):
    _chk(x, f32, nm)
  _chk(g_T_a, bf16, 'g_T_a')
  _chk(g_T_b, bf16, 'g_T_b', allow_none=True)
  B, n1 = tdist.shape
  n = n1 - 1
  ld = g_T_a.stride(0)
  assert g_T_a.shape[0] == 3 * B * n and (g_T_b is None or (g_T_b.shape[0] == 3 * B * n and g_T_b.stride(0) == ld))
  assert g_t0.numel() == B * n and g_t1.numel() == B * n
  cfg = _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg)
  L.check(lib().mnr_cast_rays_ipe_tangent_bwd(C.byref(cfg), B, n, _ptr(tdist), _ptr(origins), _ptr(directions), _ptr(radii),
                                              _ptr(basis), _ptr(g_T_a), _ptr(g_T_b), ld, _ptr(g_t0), _ptr(g_t1), _stream()))
  return g_t0, g_t1


def sdist_bwd(sdist, near, far, raydist_fn, *, B_valid=None, g_x=None, raw_density=None, density_noise=None, density_noise_std=0.0,
              density_bias=0.0, density_act='softplus', dirs=None, g_t0=None, g_t1=None, distortion_mult=0.0, weights=None,
              g_sdist_in=None, out=None):
  """d loss / d sdist [B, n+1] of one level (Model.stop_level_grad = False): see mnr_sdist_bwd in include/mnerf.h."""
  _chk(sdist, f32, 'sdist')
  B, n1 = sdist.shape
  n = n1 - 1
  for x, nm in ((near, 'near'), (far, 'far')):
    _chk(x, f32, nm)
  for x, nm in ((g_x, 'g_x'), (raw_density, 'raw_density'), (density_noise, 'density_noise'), (dirs, 'dirs'), (g_t0, 'g_t0'),
                (g_t1, 'g_t1'), (weights, 'weights'), (g_sdist_in, 'g_sdist_in')):
    _chk(x, f32, nm, allow_none=True)
  assert near.numel() == B and far.numel() == B
  assert g_x is None or (g_x.numel() == B * n and raw_density is not None and raw_density.numel() == B * n and dirs is not None)
  assert g_sdist_in is None or g_sdist_in.shape == (B, n1)
  if out is None:
    out = torch.empty((B, n1), dtype=f32, device=sdist.device)
  _chk(out, f32, 'out')
  a = L.SdistBwdArgs()
  a.B, a.B_valid, a.n = B, (B if B_valid is None else int(B_valid)), n
  a.sdist, a.near, a.far, a.raydist_fn = _ptr(sdist), _ptr(near), _ptr(far), L.RAYDIST[raydist_fn]
  a.g_x, a.raw_density, a.density_noise = _ptr(g_x), _ptr(raw_density), _ptr(density_noise)
  a.density_noise_std, a.density_bias, a.density_act = float(density_noise_std), float(density_bias), L.ACT[density_act]
  a.dirs, a.g_t0, a.g_t1 = _ptr(dirs), _ptr(g_t0), _ptr(g_t1)
  a.distortion_mult, a.weights = float(distortion_mult), _ptr(weights)
  a.g_sdist_in, a.g_sdist = _ptr(g_sdist_in), _ptr(out)
  L.check(lib().mnr_sdist_bwd(C.byref(a), _stream()))
  return out


def viewdir_enc_fill(viewdirs, n, deg_view, dst, col0, col_end):
  _chk(viewdirs, f32, 'viewdirs')
  _chk(dst, bf16, 'dst')
  B = viewdirs.shape[0]
  assert dst.shape[0] == B * n
  L.check(lib().mnr_viewdir_enc_fill(B, n, _ptr(viewdirs), deg_view, _ptr(dst), dst.stride(0), col0, col_end,
                                     _stream()))


# ----------------------------------------------------------------------------- dense


def glo_fill(table, cam_idx, B, n, dst, col0):
  """cam_idx None == zero_glo."""
  _chk(table, f32, 'table')
  _chk(cam_idx, torch.int32, 'cam_idx', allow_none=True)
  _chk(dst, bf16, 'dst')
  E, G = table.shape
  L.check(lib().mnr_glo_fill(B, n, G, _ptr(table), _ptr(cam_idx), E, _ptr(dst), dst.stride(0), col0, _stream()))


def glo_bwd(g_a, g_b, cam_idx, B, n, grad_table, num_embeddings, G):
  _chk(g_a, f32, 'g_a')
  _chk(g_b, f32, 'g_b', allow_none=True)
  _chk(cam_idx, torch.int32, 'cam_idx')
  _chk(grad_table, f32, 'grad_table')
  L.check(lib().mnr_glo_bwd(B, n, G, _ptr(g_a), _ptr(g_b), _ptr(cam_idx), num_embeddings, _ptr(grad_table), _stream()))


LAYOUT_ROWMAJOR, LAYOUT_PANEL = 0, 1      # include/mnerf.h MNR_LAYOUT_*


def to_panel(x):
  """Row-major [M, W] -> the same storage in MNR_LAYOUT_PANEL (include/mnerf.h): 1-KiB blocks of 32 rows x 16 columns,
  element (m, n) at ((m // 32) * (W // 16) + n // 16) * 512 + (m % 32) * 16 + n % 16.  Layout conversions are for tests and
  tools: on the product path every producer and consumer of a panel matrix is one of the library's own GEMMs."""
  M, W = x.shape
  assert M % 32 == 0 and W % 16 == 0
  return x.reshape(M // 32, 32, W // 16, 16).permute(0, 2, 1, 3).contiguous().view(M, W)


def from_panel(x):
  """Inverse of `to_panel`."""
  M, W = x.shape
  assert M % 32 == 0 and W % 16 == 0
  return x.reshape(M // 32, W // 16, 32, 16).permute(0, 2, 1, 3).contiguous().view(M, W)


def bits_to_tile_order(bits, N):
  """Row-major 1-bit masks [M, N/8] (bit n & 7 of byte [m, n // 8]) -> the TILE order of a panel-result GEMM (include/mnerf.h:
  8 KiB per 256 x 256 tile, 16 bytes per thread); returns a flat uint8 tensor of M * N / 8 bytes.  Tests / tools only."""
  M = bits.shape[0]
  assert M % 256 == 0 and N % 256 == 0 and bits.shape[1] == N // 8
  # row = (mt, wm, i, r), byte column = (nt, wn, j, h, kh)   ->   (mt, nt, wm, wn, kh, r, j, i, h)
  v = bits.reshape(M // 256, 2, 4, 32, N // 256, 4, 2, 2, 2)
  return v.permute(0, 4, 1, 5, 8, 3, 6, 2, 7).contiguous().view(-1)


def bits_from_tile_order(tile_bits, M, N):
  """Inverse of `bits_to_tile_order`: -> [M, N/8]."""
  v = tile_bits.reshape(M // 256, N // 256, 2, 4, 2, 32, 2, 4, 2)      # (mt, nt, wm, wn, kh, r, j, i, h)
  return v.permute(0, 2, 7, 5, 1, 3, 6, 8, 4).contiguous().view(M, N // 8)


def gemm_nt(A1, Bt, *, M, N, K1, A2=None, K2=0, lda1=None, lda2=None, ldb=None, bias=None, n_bias=0,
            relu=False, mask=None, ldmask=0, Cb=None, ldcb=0, nb=0, Cf=None, ldcf=0, f0=0, nf=0,
            bits_out=None, bits_in=None, bits_row_mod=0, a1_layout=LAYOUT_ROWMAJOR, c_layout=LAYOUT_ROWMAJOR,
            vcol=None, vcol_out=None, vcol_bias=None, walk_descending=False, max_wgs=0):
  """C[M,N] = epilogue([A1|A2] @ Bt^T).  Pointers may be views with explicit leading dimensions.  a1_layout / c_layout:
  LAYOUT_PANEL for the wide trunk's activations and gradients (include/mnerf.h; the bits are then in tile order)."""
  _chk(A1, bf16, 'A1')
  _chk(Bt, bf16, 'Bt')
  _chk(A2, bf16, 'A2', allow_none=True)
  _chk(mask, bf16, 'mask', allow_none=True)
  _chk(bias, f32, 'bias', allow_none=True)
  _chk(Cb, bf16, 'Cb', allow_none=True)
  _chk(Cf, f32, 'Cf', allow_none=True)
  a = L.GemmNTArgs()
  a.A1, a.lda1, a.K1 = A1.data_ptr(), lda1 if lda1 else A1.stride(0), K1
  a.A2, a.lda2, a.K2 = (A2.data_ptr() if A2 is not None else None), (lda2 if lda2 else (A2.stride(0) if A2 is not None else 0)), K2
  a.Bt, a.ldb = Bt.data_ptr(), ldb if ldb else Bt.stride(0)
  a.M, a.N = M, N
  a.bias, a.n_bias, a.relu = (bias.data_ptr() if bias is not None else None), n_bias, int(relu)
  a.mask, a.ldmask = (mask.data_ptr() if mask is not None else None), ldmask
  a.Cb, a.ldcb, a.nb = (Cb.data_ptr() if Cb is not None else None), ldcb, nb
  a.Cf, a.ldcf, a.f0, a.nf = (Cf.data_ptr() if Cf is not None else None), ldcf, f0, nf
  for t_, nm_ in ((bits_out, 'bits_out'), (bits_in, 'bits_in')):
    _chk(t_, torch.uint8, nm_, allow_none=True)
  a.mask_bits_out, a.ld_bits_out = (bits_out.data_ptr(), bits_out.stride(0)) if bits_out is not None else (None, 0)
  a.mask_bits_in, a.ld_bits_in = (bits_in.data_ptr(), bits_in.stride(0)) if bits_in is not None else (None, 0)
  a.bits_row_mod = bits_row_mod
  a.a1_layout, a.c_layout = a1_layout, c_layout
  a.walk_descending = int(bool(walk_descending))
  a.max_wgs = int(max_wgs)
  _chk(vcol, bf16, 'vcol', allow_none=True)
  _chk(vcol_out, f32, 'vcol_out', allow_none=True)
  assert (vcol is None) == (vcol_out is None)
  _chk(vcol_bias, f32, 'vcol_bias', allow_none=True)
  a.vcol, a.vcol_out = (vcol.data_ptr() if vcol is not None else None), (vcol_out.data_ptr() if vcol_out is not None else None)
  a.vcol_bias = vcol_bias.data_ptr() if vcol_bias is not None else None
  _e = PROFILE.start()
  L.check(lib().mnr_gemm_nt_bf16(C.byref(a), _stream()))
  PROFILE.stop(_e)


def gemm_tn(A, B, Cout, *, M, K, N, lda=None, ldb=None, ldc=None, k_valid=None, n_valid=None, bias_out=None,
            bias_n_valid=0, gcol=None, gcol_out=None, a_layout=LAYOUT_ROWMAJOR, b_layout=LAYOUT_ROWMAJOR, m_interleave=False,
            max_wgs=0, rank1=None):
  """Cout[k,n] += sum_m A[m,k] B[m,n]; optionally bias_out[n] += sum_m B[m,n] (fused bias gradient) and
  gcol_out[k] += sum_m A[m,k] gcol[m] (one more column of B given as a contiguous bf16 vector [M]).
  rank1 = (g [M] fp32, w [N] fp32, bits [M, N / 8] uint8) with B = None: B[m,n] = bit ? bf16(g[m] w[n]) : 0 is built inside
  the kernel (the proposal MLP's last dY, mnr_gemm_tn_args.rank1_*)."""
  _chk(bias_out, f32, 'bias_out', allow_none=True)
  _chk(gcol, bf16, 'gcol', allow_none=True)
  _chk(gcol_out, f32, 'gcol_out', allow_none=True)
  assert (gcol is None) == (gcol_out is None) and (gcol is None or (gcol.numel() == M and gcol.is_contiguous()))
  _chk(A, bf16, 'A')
  _chk(B, bf16, 'B', allow_none=rank1 is not None)
  _chk(Cout, f32, 'C')
  a = L.GemmTNArgs()
  a.A, a.lda, a.K = A.data_ptr(), lda if lda else A.stride(0), K
  if rank1 is not None:
    g, w, bits = rank1
    _chk(g, f32, 'rank1 g')
    _chk(w, f32, 'rank1 w')
    _chk(bits, torch.uint8, 'rank1 bits')
    assert B is None and g.numel() == M and g.is_contiguous() and w.numel() >= N and w.is_contiguous()
    assert bits.dim() == 2 and bits.shape[0] == M and bits.shape[1] * 8 >= N and bits.stride(1) == 1
    a.B, a.ldb, a.N = None, N, N
    a.rank1_g, a.rank1_w, a.rank1_bits, a.ld_rank1_bits = g.data_ptr(), w.data_ptr(), bits.data_ptr(), bits.stride(0)
  else:
    a.B, a.ldb, a.N = B.data_ptr(), ldb if ldb else B.stride(0), N
  a.M = M
  a.C, a.ldc = Cout.data_ptr(), ldc if ldc else Cout.stride(0)
  a.k_valid = K if k_valid is None else k_valid
  a.n_valid = N if n_valid is None else n_valid
  a.bias_out = bias_out.data_ptr() if bias_out is not None else None
  a.bias_n_valid = bias_n_valid
  a.gcol = gcol.data_ptr() if gcol is not None else None
  a.gcol_out = gcol_out.data_ptr() if gcol_out is not None else None
  a.a_layout, a.b_layout = a_layout, b_layout
  a.m_interleave, a.max_wgs = int(bool(m_interleave)), int(max_wgs)
  _e = PROFILE.start()
  L.check(lib().mnr_gemm_tn_bf16(C.byref(a), _stream()))
  PROFILE.stop(_e)


def mlp_chain_fwd(feat, K0, layers, *, M, W, w_head=None, b_head=None, head_out=None, acts=None, bits=None, skip_layer=0):
  """Fused Dense + ReLU chain with a Dense(1) head (csrc/fused_mlp.hip): `layers` = [(Bt [W, ldb] bf16, bias [W] fp32)],
  layer 0 reading feat [M, ld_feat] over K0 columns.  acts / bits: optional per-layer outputs (training)."""
  depth = len(layers)
  if not 1 <= depth <= L.CHAIN_MAX_DEPTH:
    raise ValueError(f'mlp_chain_fwd: depth {depth}')
  _chk(feat, bf16, 'feat')
  _chk(w_head, bf16, 'w_head', allow_none=True)
  _chk(b_head, f32, 'b_head', allow_none=True)
  _chk(head_out, f32, 'head_out', allow_none=True)
  a = L.MlpChainFwdArgs()
  a.M, a.W, a.depth, a.skip_layer = M, W, depth, int(skip_layer)
  a.feat, a.ld_feat, a.K0 = feat.data_ptr(), feat.stride(0), K0
  for i, (Bt, bias) in enumerate(layers):
    _chk(Bt, bf16, f'Bt[{i}]')
    _chk(bias, f32, f'bias[{i}]')
    assert Bt.shape[0] >= W and bias.numel() == W
    a.Bt[i], a.ldb[i], a.bias[i] = Bt.data_ptr(), Bt.stride(0), bias.data_ptr()
    if acts is not None and acts[i] is not None:
      _chk(acts[i], bf16, f'acts[{i}]')
      assert acts[i].shape == (M, W)
      a.acts[i] = acts[i].data_ptr()
    if bits is not None and bits[i] is not None:
      _chk(bits[i], torch.uint8, f'bits[{i}]')
      assert bits[i].shape == (M, W // 8)
      a.bits[i] = bits[i].data_ptr()
  if w_head is not None:
    assert w_head.numel() >= W and head_out is not None and head_out.numel() == M
    a.w_head, a.head_out = w_head.data_ptr(), head_out.data_ptr()
    a.b_head = b_head.data_ptr() if b_head is not None else None
  _e = PROFILE.start()
  L.check(lib().mnr_mlp_chain_fwd(C.byref(a), _stream()))
  PROFILE.stop(_e)


def mlp_chain_fwd_ipe(tdist, origins, directions, radii, basis, layers, *, M, W, ray_shape, warp_contract, min_deg,
                      max_deg, disable_integration=False, w_head=None, b_head=None, head_out=None, act_last=None):
  """The inference chain with layer 0's IPE features produced in the kernel (csrc/fused_mlp.hip, mnr_mlp_chain_fwd_ipe):
  no feature matrix.  layers[0][0] is the group-major reordered kernel^T (include/mnerf.h); tdist [B, n+1] with B*n = M."""
  depth = len(layers)
  if not 1 <= depth <= L.CHAIN_MAX_DEPTH:
    raise ValueError(f'mlp_chain_fwd_ipe: depth {depth}')
  for x, nm in ((tdist, 'tdist'), (origins, 'origins'), (directions, 'directions'), (radii, 'radii'), (basis, 'basis')):
    _chk(x, f32, nm)
  _chk(w_head, bf16, 'w_head', allow_none=True)
  _chk(b_head, f32, 'b_head', allow_none=True)
  _chk(head_out, f32, 'head_out', allow_none=True)
  B, n1 = tdist.shape
  assert B * (n1 - 1) == M and origins.shape[0] == B and directions.shape[0] == B and radii.numel() == B
  a = L.MlpChainFwdArgs()
  a.M, a.W, a.depth, a.skip_layer = M, W, depth, 0
  for i, (Bt, bias) in enumerate(layers):
    _chk(Bt, bf16, f'Bt[{i}]')
    _chk(bias, f32, f'bias[{i}]')
    assert Bt.shape[0] >= W and bias.numel() == W
    a.Bt[i], a.ldb[i], a.bias[i] = Bt.data_ptr(), Bt.stride(0), bias.data_ptr()
  if act_last is not None:
    _chk(act_last, bf16, 'act_last')
    assert act_last.shape == (M, W)
    a.acts[depth - 1] = act_last.data_ptr()
  if w_head is not None:
    assert w_head.numel() >= W and head_out is not None and head_out.numel() == M
    a.w_head, a.head_out = w_head.data_ptr(), head_out.data_ptr()
    a.b_head = b_head.data_ptr() if b_head is not None else None
  q = L.ChainIpeArgs()
  q.cfg = _ipe_cfg(ray_shape, warp_contract, disable_integration, basis, min_deg, max_deg)
  q.n = n1 - 1
  q.tdist, q.origins, q.directions, q.radii, q.basis = _ptr(tdist), _ptr(origins), _ptr(directions), _ptr(radii), _ptr(basis)
  _e = PROFILE.start()
  L.check(lib().mnr_mlp_chain_fwd_ipe(C.byref(a), C.byref(q), _stream()))
  PROFILE.stop(_e)


def mlp_chain_bwd(g_head, w_head, bits, Bws, dYs, *, M, W, dY_in=None):
  """The dX chain of the fused Dense stack: dY[last] = mask * (g_head (x) w_head), dY[i-1] = mask_{i-1} * (dY[i] W_i^T).
  Bws[i] (i >= 1): [W, ldb] bf16 kernel as stored (rows = inputs); Bws[0] unused."""
  depth = len(bits)
  assert len(dYs) == depth and len(Bws) == depth
  a = L.MlpChainBwdArgs()
  a.M, a.W, a.depth = M, W, depth
  if dY_in is not None:
    _chk(dY_in, bf16, 'dY_in')
    assert dY_in.shape == (M, W) and dYs[depth - 1] is None
    a.dY_in = dY_in.data_ptr()
  else:
    _chk(g_head, f32, 'g_head')
    _chk(w_head, f32, 'w_head')
    assert g_head.numel() == M and w_head.numel() == W
    a.g_head, a.w_head = g_head.data_ptr(), w_head.data_ptr()
  for i in range(depth):
    _chk(bits[i], torch.uint8, f'bits[{i}]')
    assert bits[i].shape == (M, W // 8)
    a.bits[i] = bits[i].data_ptr()
    if dYs[i] is not None:
      _chk(dYs[i], bf16, f'dY[{i}]')
      assert dYs[i].shape == (M, W)
      a.dY[i] = dYs[i].data_ptr()
    if i >= 1:
      _chk(Bws[i], bf16, f'Bw[{i}]')
      a.Bw[i], a.ldb[i] = Bws[i].data_ptr(), Bws[i].stride(0)
  _e = PROFILE.start()
  L.check(lib().mnr_mlp_chain_bwd(C.byref(a), _stream()))
  PROFILE.stop(_e)


def colsum(X, M, n_valid, out, ld=None):
  _chk(X, bf16, 'X')
  _chk(out, f32, 'out')
  L.check(lib().mnr_colsum_bf16(_ptr(X), ld if ld else X.stride(0), M, n_valid, _ptr(out), _stream()))


def pack_weights(params, descs_dev, n_desc, max_elems, dst):
  _chk(params, f32, 'params')
  _chk(dst, bf16, 'dst')
  L.check(lib().mnr_pack_weights_bf16(_ptr(params), _ptr(descs_dev), n_desc, max_elems, _ptr(dst), _stream()))


def scatter_add(src, ld_src, row0, col0, rows, cols, dst, ld_dst):
  _chk(src, f32, 'src')
  _chk(dst, f32, 'dst')
  L.check(lib().mnr_scatter_add_f32(_ptr(src), ld_src, row0, col0, rows, cols, _ptr(dst), ld_dst, _stream()))


def cast_f32_to_bf16(src, ld_src, M, n, dst, ld_dst, col0):
  _chk(src, f32, 'src')
  _chk(dst, bf16, 'dst')
  L.check(lib().mnr_cast_f32_to_bf16(_ptr(src), ld_src, M, n, _ptr(dst), ld_dst, col0, _stream()))


def act_fwd(kind, z, a):
  """a = act(z) for a non-ReLU net_activation ('softplus' | 'silu'); z, a contiguous bf16 of the same shape."""
  _chk(z, bf16, 'z')
  _chk(a, bf16, 'a')
  assert z.shape == a.shape
  L.check(lib().mnr_act_fwd_bf16(L.NET_ACT[kind], z.numel(), _ptr(z), _ptr(a), _stream()))


def act_bwd(kind, z, d):
  """d *= act'(z) in place: gradient w.r.t. the activation -> w.r.t. the pre-activation."""
  _chk(z, bf16, 'z')
  _chk(d, bf16, 'd')
  assert z.shape == d.shape
  L.check(lib().mnr_act_bwd_bf16(L.NET_ACT[kind], z.numel(), _ptr(z), _ptr(d), _stream()))


def act_tangent_fwd(kind, z, U, T):
  """T = act'(z) * U: the tangent network of the density-gradient normals behind a non-ReLU activation; z [M, W], U, T [3M, W]."""
  for x, nm in ((z, 'z'), (U, 'U'), (T, 'T')):
    _chk(x, bf16, nm)
  assert U.shape == T.shape and U.numel() == 3 * z.numel()
  L.check(lib().mnr_act_tangent_fwd_bf16(L.NET_ACT[kind], z.numel(), _ptr(z), _ptr(U), _ptr(T), _stream()))


def act_tangent_bwd(kind, z, U, G, extra):
  """G (d loss / d T, [3M, W]) *= act'(z) in place; extra [M, W] = sum_c G_c * U_c * act''(z) (joins the primal gradient of z)."""
  for x, nm in ((z, 'z'), (U, 'U'), (G, 'G'), (extra, 'extra')):
    _chk(x, bf16, nm)
  assert U.shape == G.shape and U.numel() == 3 * z.numel() and extra.shape == z.shape
  L.check(lib().mnr_act_tangent_bwd_bf16(L.NET_ACT[kind], z.numel(), _ptr(z), _ptr(U), _ptr(G), _ptr(extra), _stream()))


def add_noise_bf16(X, cols, noise, scale):
  """X[:, :cols] += scale * noise (fp32 add, one bf16 rounding); X bf16 [M, ld], noise fp32 [M, cols]."""
  _chk(noise, f32, 'noise')
  if X.dtype != act_dtype() or not _on_device(X):
    raise ValueError(f'X must be a {act_dtype()} device tensor')
  M = X.shape[0]
  assert noise.shape == (M, cols)
  L.check(lib().mnr_add_noise_bf16(M, cols, _ptr(X), X.stride(0), _ptr(noise), float(scale), _stream()))


_HEAD_SCRATCH = {}


def _head_scratch(device):
  """Workspace for the per-workgroup dW / db partials of mnr_small_head_bwd (4 MiB per device AND stream, allocated
  once: two levels' backward passes may run side by side on different streams, multinerf_amd/streams.py)."""
  key = (device, getattr(_stream(), 'value', None))
  t = _HEAD_SCRATCH.get(key)
  if t is None:
    t = _HEAD_SCRATCH[key] = torch.empty(1 << 20, dtype=f32, device=device)
  return t


def small_head_bwd(H, ldh, g, W, *, M, K, Cn, dX=None, lddx=0, relu_mask=True, dW=None, db=None, bits=None,
                   bits_row_mod=0):
  _chk(bits, torch.uint8, 'bits', allow_none=True)
  _chk(H, bf16, 'H')
  _chk(g, f32, 'g')
  _chk(W, f32, 'W')
  _e = PROFILE.start()
  scratch = _head_scratch(H.device)
  L.check(lib().mnr_small_head_bwd(M, K, Cn, _ptr(H), ldh, _ptr(g), _ptr(W), _ptr(dX), lddx, int(relu_mask),
                                   _ptr(dW), _ptr(db), _ptr(bits), bits.stride(0) if bits is not None else 0,
                                   bits_row_mod, _ptr(scratch), scratch.numel(), _stream()))
  PROFILE.stop(_e, 'small_head_bwd', 2 * M * K * (2 if dX is not None else 1) + 4 * M * Cn)


# ----------------------------------------------------------------------------- compositing


def composite_cfg(n, *, opaque_background, density_act, density_bias, density_noise_std, has_rgb, rgb_act,
                  rgb_premultiplier, rgb_bias, rgb_padding, bg_mode, bg_value):
  return L.CompositeCfg(n, int(opaque_background), L.ACT[density_act], float(density_bias),
                        float(density_noise_std), int(has_rgb), L.ACT[rgb_act], float(rgb_premultiplier),
                        float(rgb_bias), float(rgb_padding), int(bg_mode), float(bg_value))


def composite_fwd(cfg, raw_density, tdist, dirs, *, raw_rgb=None, density_noise=None, bg=None,
                  exposure_scale=None, want_acc=True):
  _chk(raw_density, f32, 'raw_density')
  _chk(tdist, f32, 'tdist')
  _chk(dirs, f32, 'dirs')
  for x, nm in ((raw_rgb, 'raw_rgb'), (density_noise, 'density_noise'), (bg, 'bg'),
                (exposure_scale, 'exposure_scale')):
    _chk(x, f32, nm, allow_none=True)
  B, n = raw_density.shape
  dev = raw_density.device
  density = torch.empty((B, n), dtype=f32, device=dev)
  weights = torch.empty((B, n), dtype=f32, device=dev)
  rgb = torch.empty((B, n, 3), dtype=f32, device=dev) if cfg.has_rgb else None
  rgb_out = torch.empty((B, 3), dtype=f32, device=dev)
  acc = torch.empty((B,), dtype=f32, device=dev) if want_acc else None
  _e = PROFILE.start()
  L.check(lib().mnr_composite_fwd(C.byref(cfg), B, _ptr(raw_density), _ptr(density_noise), _ptr(raw_rgb),
                                  _ptr(tdist), _ptr(dirs), _ptr(bg), _ptr(exposure_scale), _ptr(density),
                                  _ptr(rgb), _ptr(weights), _ptr(rgb_out), _ptr(acc), _stream()))
  PROFILE.stop(_e, 'composite_fwd', 4 * (raw_density.numel() * (2 + 2 + (6 if raw_rgb is not None else 0))))
  return density, rgb, weights, rgb_out, acc


def composite_bwd(cfg, raw_density, tdist, dirs, weights, *, raw_rgb=None, density_noise=None, bg=None,
                  exposure_scale=None, g_rgb_out=None, g_weights=None, g_den_bf16=None, ld_bf16=0,
                  want_f32=True, g_exposure_scale=None, losses=None, g_raw_density_out=None, g_x_out=None):
  """Compositing VJP; with `losses` the level's training losses are fused in front of it (mnr_level_bwd):
  g_raw_density_out: optional [B, n] fp32 destination for d loss / d raw_density (else a fresh tensor).
  g_x_out: optional [B, n] fp32 destination for d loss / d (sigma * delta) (Model.stop_level_grad = False, mnr_sdist_bwd).
  losses = dict(B_valid=..., data=dict(type, charb_padding, mult, rgb_out, gt, lossmult, denom, stats) | None,
                weights=dict(mode='interlevel'|'distortion', mult, sdist, t_ref, w_ref, stat) | None)."""
  B, n = raw_density.shape
  dev = raw_density.device
  for x, nm in ((raw_density, 'raw_density'), (tdist, 'tdist'), (dirs, 'dirs'), (weights, 'weights')):
    _chk(x, f32, nm)
  for x, nm in ((g_rgb_out, 'g_rgb_out'), (g_weights, 'g_weights')):
    _chk(x, f32, nm, allow_none=True)
  _chk(g_den_bf16, bf16, 'g_den_bf16', allow_none=True)
  if g_raw_density_out is not None:
    _chk(g_raw_density_out, f32, 'g_raw_density_out')
    assert want_f32 and g_raw_density_out.shape == (B, n) and g_raw_density_out.is_contiguous()
    g_raw_density = g_raw_density_out
  else:
    g_raw_density = torch.empty((B, n), dtype=f32, device=dev) if want_f32 else None
  g_raw_rgb = torch.empty((B, n, 3), dtype=f32, device=dev) if cfg.has_rgb else None
  a = L.LevelBwdArgs()
  a.cfg = cfg
  a.B = B
  a.B_valid = B if losses is None else int(losses['B_valid'])
  p = lambda t: None if t is None else t.data_ptr()
  a.raw_density, a.density_noise, a.raw_rgb, a.tdist, a.dirs = p(raw_density), p(density_noise), p(raw_rgb), p(tdist), p(dirs)
  a.bg, a.exposure_scale, a.weights, a.g_rgb_out, a.g_weights = p(bg), p(exposure_scale), p(weights), p(g_rgb_out), p(g_weights)
  a.g_raw_density, a.g_raw_density_bf16, a.ld_bf16 = p(g_raw_density), p(g_den_bf16), ld_bf16
  a.g_raw_rgb, a.g_exposure_scale = p(g_raw_rgb), p(g_exposure_scale)
  a.data_loss_type, a.wloss_mode = -1, 0
  if g_x_out is not None:
    _chk(g_x_out, f32, 'g_x_out')
    assert g_x_out.shape == (B, n) and g_x_out.is_contiguous()
    a.g_x = p(g_x_out)
  keep = []
  if losses is not None and losses.get('data') is not None:
    d = losses['data']
    if d['type'] not in L.DATA_LOSS:
      raise ValueError(f"unsupported data_loss_type {d['type']!r}")
    for k in ('rgb_out', 'gt', 'lossmult', 'denom', 'stats'):
      _chk(d[k], f32, 'data.' + k)
    assert d['rgb_out'].shape[0] == B and d['gt'].shape[0] == B and d['lossmult'].shape[0] == B
    a.data_loss_type, a.charb_padding, a.data_loss_mult = L.DATA_LOSS[d['type']], float(d['charb_padding']), float(d['mult'])
    a.rgb_out, a.gt, a.lossmult, a.lm_c = p(d['rgb_out']), p(d['gt']), p(d['lossmult']), d['lossmult'].shape[-1]
    a.denom, a.data_stats = p(d['denom']), p(d['stats'])
    keep.append(d)
  if losses is not None and losses.get('weights') is not None:
    w = losses['weights']
    _chk(w['sdist'], f32, 'weights.sdist')
    _chk(w['stat'], f32, 'weights.stat')
    assert w['sdist'].shape == (B, n + 1)
    a.wloss_mult, a.sdist, a.wloss_stat = float(w['mult']), p(w['sdist']), p(w['stat'])
    if w['mode'] == 'interlevel':
      _chk(w['t_ref'], f32, 'weights.t_ref')
      _chk(w['w_ref'], f32, 'weights.w_ref')
      assert w['t_ref'].shape[0] == B and w['t_ref'].shape[1] == w['w_ref'].shape[1] + 1
      a.wloss_mode, a.n_ref, a.t_ref, a.w_ref = 1, w['w_ref'].shape[1], p(w['t_ref']), p(w['w_ref'])
    elif w['mode'] == 'distortion':
      a.wloss_mode = 2
    else:
      raise ValueError(f"weights.mode {w['mode']!r}")
    keep.append(w)
  _e = PROFILE.start()
  L.check(lib().mnr_level_bwd(C.byref(a), _stream()))
  PROFILE.stop(_e, 'composite_bwd', 4 * (raw_density.numel() * (3 + (3 if raw_rgb is not None else 0))) + (2 + (12 if raw_rgb is not None else 0)) * raw_density.numel())
  return g_raw_density, g_raw_rgb


def exposure_scale(exposure_values, exposure_idx, offsets):
  _chk(exposure_values, f32, 'exposure_values')
  _chk(exposure_idx, torch.int32, 'exposure_idx')
  _chk(offsets, f32, 'offsets', allow_none=True)
  B = exposure_values.numel()
  out = torch.empty((B, 3), dtype=f32, device=exposure_values.device)
  L.check(lib().mnr_exposure_scale(B, _ptr(exposure_values), _ptr(exposure_idx), _ptr(offsets), _ptr(out), _stream()))
  return out


def exposure_scale_bwd(exposure_values, exposure_idx, g_scale, g_offsets, B_valid):
  _chk(g_scale, f32, 'g_scale')
  _chk(g_offsets, f32, 'g_offsets')
  L.check(lib().mnr_exposure_scale_bwd(B_valid, _ptr(exposure_values), _ptr(exposure_idx), _ptr(g_scale),
                                       _ptr(g_offsets), _stream()))


def render_extras(weights, tdist, t_far):
  for x, nm in ((weights, 'weights'), (tdist, 'tdist'), (t_far, 't_far')):
    _chk(x, f32, nm)
  B, n = weights.shape
  out = torch.empty((B, 4), dtype=f32, device=weights.device)
  L.check(lib().mnr_render_extras(B, n, _ptr(weights), _ptr(tdist), _ptr(t_far), _ptr(out), _stream()))
  return out


# ----------------------------------------------------------------------------- Ref-NeRF


class IdeTablesDev:
  """Device copies of ref_utils.ide_tables(deg_view) + the C struct that points at them."""

  def __init__(self, deg_view, device):
    from multinerf_amd import ref_utils
    m, l, mat, sigma = ref_utils.ide_tables(deg_view)
    self.T = len(m)
    self.m = torch.as_tensor(m, dtype=torch.int32, device=device)
    self.l = torch.as_tensor(l, dtype=torch.int32, device=device)
    self.mat = torch.as_tensor(mat, dtype=f32, device=device).contiguous()
    self.sigma = torch.as_tensor(sigma, dtype=f32, device=device)
    self.c = L.IdeTables(self.T, mat.shape[0] - 1, self.m.data_ptr(), self.l.data_ptr(), self.sigma.data_ptr(),
                         self.mat.data_ptr())


# mnr_ref_head_fwd / _bwd feature bits (include/mnerf.h MNR_REF_*)
REF_PRED_NORMALS, REF_DENSITY_NORMALS, REF_REFLECT, REF_IDE, REF_N_DOT_V, REF_ROUGHNESS = 1, 2, 4, 8, 16, 32
REF_ALL = 63


def ref_head_fwd(small, raw_grad, viewdirs, n, tabs, roughness_bias, vi, col0, col_end, features=REF_ALL, deg_view=0):
  """-> (normals, normals_pred, roughness); None for the parts `features` switches off."""
  for x, nm in ((small, 'small'), (viewdirs, 'viewdirs')):
    _chk(x, f32, nm)
  _chk(raw_grad, f32, 'raw_grad', allow_none=True)
  _chk(vi, bf16, 'vi')
  M = small.shape[0]
  dev = small.device
  normals = torch.empty((M, 3), dtype=f32, device=dev) if features & REF_DENSITY_NORMALS else None
  npred = torch.empty((M, 3), dtype=f32, device=dev) if features & REF_PRED_NORMALS else None
  rough = torch.empty((M,), dtype=f32, device=dev) if features & REF_ROUGHNESS else None
  L.check(lib().mnr_ref_head_fwd(M, n, _ptr(small), _ptr(raw_grad), _ptr(viewdirs), C.byref(tabs.c) if tabs is not None else None,
                                 int(features), int(deg_view), float(roughness_bias), _ptr(vi), vi.stride(0), col0, col_end,
                                 _ptr(normals), _ptr(npred), _ptr(rough), _stream()))
  return normals, npred, rough


def ref_head_bwd(small, raw_grad, viewdirs, n, tabs, roughness_bias, dvi_a, dvi_b, col0, g_npred, g_n, dhb, col_gp,
                 col_rough, features=REF_ALL, deg_view=0):
  """-> g_raw_grad [3, M] (None without density-gradient normals)."""
  M = small.shape[0]
  _chk(dvi_a, bf16, 'dvi_a')
  _chk(dvi_b, bf16, 'dvi_b', allow_none=True)
  _chk(dhb, bf16, 'dhb')
  g_raw_grad = torch.empty((3, M), dtype=f32, device=small.device) if features & REF_DENSITY_NORMALS else None
  L.check(lib().mnr_ref_head_bwd(M, n, _ptr(small), _ptr(raw_grad), _ptr(viewdirs), C.byref(tabs.c) if tabs is not None else None,
                                 int(features), int(deg_view), float(roughness_bias), _ptr(dvi_a), _ptr(dvi_b), dvi_a.stride(0), col0,
                                 _ptr(g_npred), _ptr(g_n), _ptr(dhb), dhb.stride(0), col_gp, col_rough,
                                 _ptr(g_raw_grad), _stream()))
  return g_raw_grad


def add_cols_bf16(a, b, dst, cols):
  """dst[:, :cols] = a[:, :cols] + b[:, :cols] (row strides taken from the tensors)."""
  for x, nm in ((a, 'a'), (dst, 'dst')):
    if x.dtype != act_dtype() or not _on_device(x):
      raise ValueError(f'{nm} must be a {act_dtype()} device tensor')
  M = a.shape[0]
  L.check(lib().mnr_add_cols_bf16(M, cols, _ptr(a), a.stride(0), _ptr(b), b.stride(0) if b is not None else 0,
                                  _ptr(dst), dst.stride(0), _stream()))


def ref_color_fwd(raw_rgb, small, premult, rgb_bias, pad, use_tint):
  _chk(raw_rgb, f32, 'raw_rgb')
  _chk(small, f32, 'small')
  M = small.shape[0]
  out = torch.empty((M, 3), dtype=f32, device=small.device)
  L.check(lib().mnr_ref_color_fwd(M, _ptr(raw_rgb), _ptr(small), float(premult), float(rgb_bias), float(pad),
                                  int(use_tint), _ptr(out), _stream()))
  return out


def ref_color_bwd(raw_rgb, small, premult, rgb_bias, pad, use_tint, g_rgb, dhb, col_diffuse, col_tint):
  _chk(g_rgb, f32, 'g_rgb')
  _chk(dhb, bf16, 'dhb')
  M = small.shape[0]
  g_raw_rgb = torch.empty((M, 3), dtype=f32, device=small.device)
  L.check(lib().mnr_ref_color_bwd(M, _ptr(raw_rgb), _ptr(small), float(premult), float(rgb_bias), float(pad),
                                  int(use_tint), _ptr(g_rgb), _ptr(g_raw_rgb), _ptr(dhb), dhb.stride(0), col_diffuse,
                                  col_tint, _stream()))
  return g_raw_rgb


def density_normals_fwd(raw_grad):
  """normals = -l2_normalize(raw_grad) (models.py:492); raw_grad [3, M] component-major."""
  _chk(raw_grad, f32, 'raw_grad')
  M = raw_grad.shape[1]
  out = torch.empty((M, 3), dtype=f32, device=raw_grad.device)
  L.check(lib().mnr_density_normals_fwd(M, _ptr(raw_grad), _ptr(out), _stream()))
  return out


def density_normals_bwd(raw_grad, g_normals):
  _chk(raw_grad, f32, 'raw_grad')
  _chk(g_normals, f32, 'g_normals')
  M = raw_grad.shape[1]
  out = torch.empty((3, M), dtype=f32, device=raw_grad.device)
  L.check(lib().mnr_density_normals_bwd(M, _ptr(raw_grad), _ptr(g_normals), _ptr(out), _stream()))
  return out


def pred_normals_fwd(small, col):
  """normals_pred = -l2_normalize(small[:, col:col+3]) (models.py:498)."""
  _chk(small, f32, 'small')
  M, ld = small.shape
  out = torch.empty((M, 3), dtype=f32, device=small.device)
  L.check(lib().mnr_pred_normals_fwd(M, _ptr(small), ld, col, _ptr(out), _stream()))
  return out


def pred_normals_bwd(small, col, g_npred, dhb, col_g):
  _chk(small, f32, 'small')
  _chk(g_npred, f32, 'g_npred')
  _chk(dhb, bf16, 'dhb')
  M, ld = small.shape
  L.check(lib().mnr_pred_normals_bwd(M, _ptr(small), ld, col, _ptr(g_npred), _ptr(dhb), dhb.stride(0), col_g, _stream()))


def ref_losses(mult_o, mult_p, target_is_pred, weights, normals, npred, viewdirs, stats, g_w, want_grad, *, B_valid):
  for x, nm in ((weights, 'weights'), (viewdirs, 'viewdirs'), (stats, 'stats')):
    _chk(x, f32, nm)
  _chk(normals, f32, 'normals', allow_none=True)
  _chk(npred, f32, 'npred', allow_none=True)
  B, n = weights.shape
  g_n = torch.zeros_like(normals) if (want_grad and normals is not None) else None
  g_np = torch.zeros_like(npred) if (want_grad and npred is not None) else None
  L.check(lib().mnr_ref_losses(B_valid, n, float(mult_o), float(mult_p), int(target_is_pred), _ptr(weights),
                               _ptr(normals), _ptr(npred), _ptr(viewdirs), _ptr(stats), _ptr(g_w), _ptr(g_n),
                               _ptr(g_np), _stream()))
  return g_n, g_np


def weighted_sum(weights, values):
  _chk(weights, f32, 'weights')
  _chk(values, f32, 'values')
  B, n = weights.shape
  Cn = values.numel() // (B * n)
  out = torch.empty((B, Cn), dtype=f32, device=weights.device)
  L.check(lib().mnr_weighted_sum(B, n, Cn, _ptr(weights), _ptr(values), _ptr(out), _stream()))
  return out


# ----------------------------------------------------------------------------- losses


def lossmult_sum(lossmult, B_valid, out):
  _chk(lossmult, f32, 'lossmult')
  _chk(out, f32, 'out')
  L.check(lib().mnr_lossmult_sum(B_valid, _ptr(lossmult), lossmult.shape[-1], _ptr(out), _stream()))


def render_metrics(B_valid, *, distance_mean=None, disps=None, acc=None, alphas=None, normals=None, normals_gt=None,
                   out_disp=None, out_normal=None):
  for x, nm in ((distance_mean, 'distance_mean'), (disps, 'disps'), (acc, 'acc'), (alphas, 'alphas'),
                (normals, 'normals'), (normals_gt, 'normals_gt'), (out_disp, 'out_disp'), (out_normal, 'out_normal')):
    _chk(x, f32, nm, allow_none=True)
  L.check(lib().mnr_render_metrics(B_valid, _ptr(distance_mean), _ptr(disps), _ptr(acc), _ptr(alphas), _ptr(normals),
                                   _ptr(normals_gt), _ptr(out_disp), _ptr(out_normal), _stream()))


def data_loss(loss_type, charb_padding, loss_mult, rgb, gt, lossmult, denom, stats, *, B_valid, want_grad=True):
  for x, nm in ((rgb, 'rgb'), (gt, 'gt'), (lossmult, 'lossmult'), (denom, 'denom'), (stats, 'stats')):
    _chk(x, f32, nm)
  if loss_type not in L.DATA_LOSS:
    raise ValueError(f'unsupported data_loss_type {loss_type!r}')
  B = rgb.shape[0]
  g = torch.empty_like(rgb) if want_grad else None
  L.check(lib().mnr_data_loss(L.DATA_LOSS[loss_type], float(charb_padding), float(loss_mult), B, B_valid,
                              _ptr(rgb), _ptr(gt), _ptr(lossmult), lossmult.shape[-1], _ptr(denom),
                              _ptr(stats), _ptr(g), _stream()))
  return g


def robustnerf_mask(rgb, gt, lossmult, loss_threshold, *, B_valid, patch_size, inner_patch_size, filter_size,
                    smoothed_inlier_quantile, inner_patch_inlier_quantile, enable=True, mask=None, lossmult_out=None,
                    err=None, stats=None, mse=None, denom=None):
  """robustnerf.robustnerf_mask (robustnerf.py:23-86) for one level: rgb, gt [B,3], lossmult [B,1|3], loss_threshold a
  device scalar; the first B_valid rays are [patch][y][x] pixels.  Returns (mask [B], lossmult * mask [B,lm_c]); `err`
  [B] receives the per-pixel error, `stats` [4] += the means the reference logs, `mse` [1] += the level's mse over `denom`
  with the unmasked lossmult.  Enqueues one launch, reads nothing back."""
  for x, nm in ((rgb, 'rgb'), (gt, 'gt'), (lossmult, 'lossmult'), (loss_threshold, 'loss_threshold')):
    _chk(x, f32, nm)
  for x, nm in ((mask, 'mask'), (lossmult_out, 'lossmult_out'), (err, 'err'), (stats, 'stats'), (mse, 'mse'), (denom, 'denom')):
    _chk(x, f32, nm, allow_none=True)
  B = rgb.shape[0]
  lm_c = lossmult.shape[-1]
  if rgb.shape != (B, 3) or gt.shape != (B, 3) or lossmult.shape != (B, lm_c):
    raise ValueError(f'robustnerf_mask: rgb {tuple(rgb.shape)}, gt {tuple(gt.shape)}, lossmult {tuple(lossmult.shape)} must be [B,3], [B,3], [B,1|3]')
  if loss_threshold.numel() != 1:
    raise ValueError('robustnerf_mask: loss_threshold must hold one value')
  if mask is None:
    mask = torch.empty((B,), dtype=f32, device=rgb.device)
  if lossmult_out is None:
    lossmult_out = torch.empty_like(lossmult)
  if mask.numel() != B or lossmult_out.shape != lossmult.shape or (err is not None and err.numel() < B_valid):
    raise ValueError('robustnerf_mask: mask [B], lossmult_out [B,lm_c] and err [B] must match the batch')
  if (stats is not None and stats.numel() < 4) or (mse is not None and (mse.numel() < 1 or denom is None)):
    raise ValueError('robustnerf_mask: stats needs 4 entries, mse one entry and denom')
  a = L.RobustArgs()
  a.B, a.B_valid = B, int(B_valid)
  a.patch_size, a.inner_patch_size, a.filter_size, a.enable = int(patch_size), int(inner_patch_size), int(filter_size), int(bool(enable))
  a.smoothed_inlier_quantile, a.inner_patch_inlier_quantile = float(smoothed_inlier_quantile), float(inner_patch_inlier_quantile)
  p = lambda t: None if t is None else t.data_ptr()
  a.rgb, a.gt, a.lossmult, a.lm_c, a.loss_threshold, a.denom = p(rgb), p(gt), p(lossmult), lm_c, p(loss_threshold), p(denom)
  a.mask, a.lossmult_out, a.err, a.stats, a.mse = p(mask), p(lossmult_out), p(err), p(stats), p(mse)
  L.check(lib().mnr_robustnerf_mask(C.byref(a), _stream()))
  return mask, lossmult_out


def quantile(x, q, out=None, *, N=None):
  """jnp.quantile(x[:N], q) into the device scalar `out` (exact order statistics, linear interpolation; no host read)."""
  _chk(x, f32, 'x')
  _chk(out, f32, 'out', allow_none=True)
  N = x.numel() if N is None else int(N)
  if N > x.numel():
    raise ValueError(f'quantile: N = {N} exceeds the {x.numel()} values of x')
  if out is None:
    out = torch.empty((1,), dtype=f32, device=x.device)
  L.check(lib().mnr_quantile(N, _ptr(x), float(q), _ptr(out), _stream()))
  return out


# ----------------------------------------------------------------------------- evaluation metrics (csrc/metrics.hip)

f64 = torch.float64


def _image_pair(a, b, name, dtypes):
  for x, nm in ((a, 'a'), (b, 'b')):
    if x is None:
      raise ValueError(f'{name}: {nm} is None')
    if not _on_device(x):
      raise ValueError(f'{name}: {nm} must be a device tensor (the HIP path has no CPU fallback)')
    if x.dtype not in dtypes:
      raise ValueError(f'{name}: {nm} must be one of {dtypes}, is {x.dtype}')
    if not x.is_contiguous():
      raise ValueError(f'{name}: {nm} must be contiguous')
  if a.dim() != 3 or a.shape != b.shape:
    raise ValueError(f'{name}: needs two [H,W,C] images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}')


def ssim(a, b, *, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, crop=0, return_map=False, out=None):
  """dm_pix.ssim(a, b) of two [H,W,C] float32 device images, over x[crop:-crop, crop:-crop] when crop > 0.  Returns the
  mean as a float64 device scalar [1] (and the [H', W', C] float32 SSIM map with return_map).  Two launches, no host read."""
  _image_pair(a, b, 'ssim', (f32,))
  _chk(out, f64, 'out', allow_none=True)
  H, W, Cn = (int(v) for v in a.shape)
  n_part = lib().mnr_ssim_partials(H, W, Cn, int(crop), int(filter_size))
  args = L.SsimArgs()
  args.H, args.W, args.C, args.crop, args.filter_size = H, W, Cn, int(crop), int(filter_size)
  args.filter_sigma, args.max_val, args.k1, args.k2 = float(filter_sigma), float(max_val), float(k1), float(k2)
  partials = torch.empty((max(n_part, 1),), dtype=f64, device=a.device)
  if out is None:
    out = torch.empty((1,), dtype=f64, device=a.device)
  smap = None
  if return_map and n_part > 0:
    smap = torch.empty((H - 2 * int(crop) - int(filter_size) + 1, W - 2 * int(crop) - int(filter_size) + 1, Cn), dtype=f32,
                       device=a.device)
  args.a, args.b, args.map, args.partials, args.out = a.data_ptr(), b.data_ptr(), None if smap is None else smap.data_ptr(), \
      partials.data_ptr(), out.data_ptr()
  L.check(lib().mnr_ssim(C.byref(args), _stream()))          # (invalid shapes / filters are reported by the library)
  return (out, smap) if return_map else out


def image_sqdiff(a, b, *, quantize=False, crop=0, q_out=None, out=None):
  """sum (q(a) - b)^2 over x[crop:-crop, crop:-crop] of two [H,W,C] device images (float32 or float64 each) as a float64
  device scalar [1]; quantize: q(a) = rint(255 a) / 255.  q_out ([H,W,C] float32) receives q(a) of the whole image."""
  _image_pair(a, b, 'image_sqdiff', (f32, f64))
  _chk(q_out, f32, 'q_out', allow_none=True)
  _chk(out, f64, 'out', allow_none=True)
  if q_out is not None and q_out.shape != a.shape:
    raise ValueError(f'image_sqdiff: q_out {tuple(q_out.shape)} must have the shape of a {tuple(a.shape)}')
  H, W, Cn = (int(v) for v in a.shape)
  args = L.SqdiffArgs()
  args.H, args.W, args.C, args.crop, args.quantize = H, W, Cn, int(crop), int(bool(quantize))
  args.a_f64, args.b_f64 = int(a.dtype == f64), int(b.dtype == f64)
  partials = torch.empty((max(lib().mnr_image_sqdiff_partials(a.numel()), 1),), dtype=f64, device=a.device)
  if out is None:
    out = torch.empty((1,), dtype=f64, device=a.device)
  args.a, args.b, args.q_out, args.partials, args.out = a.data_ptr(), b.data_ptr(), None if q_out is None else q_out.data_ptr(), \
      partials.data_ptr(), out.data_ptr()
  L.check(lib().mnr_image_sqdiff(C.byref(args), _stream()))
  return out


def cc_gram(img, ref, mask0, eps, *, write_mask0=False, out=None):
  """One colour-correction iteration's normal equations (image.color_correct, image.py:95-116): img, ref [N,3] float64,
  mask0 [N,3] uint8 (written when write_mask0).  Returns [3,65] float64 on the device: per channel the upper triangle of
  A^T A (55, row-major) and A^T b (10)."""
  _chk(img, f64, 'img')
  _chk(ref, f64, 'ref')
  _chk(mask0, torch.uint8, 'mask0')
  _chk(out, f64, 'out', allow_none=True)
  N = img.shape[0]
  if img.shape != (N, 3) or ref.shape != (N, 3) or mask0.shape != (N, 3):
    raise ValueError(f'cc_gram: img {tuple(img.shape)}, ref {tuple(ref.shape)} and mask0 {tuple(mask0.shape)} must be [N,3]')
  args = L.CcGramArgs()
  args.N, args.eps, args.write_mask0 = N, float(eps), int(bool(write_mask0))
  partials = torch.empty((max(lib().mnr_cc_gram_partials(N), 1),), dtype=f64, device=img.device)
  if out is None:
    out = torch.empty((3, L.CC_GRAM_OUT), dtype=f64, device=img.device)
  args.img, args.ref, args.mask0, args.partials, args.out = img.data_ptr(), ref.data_ptr(), mask0.data_ptr(), partials.data_ptr(), \
      out.data_ptr()
  L.check(lib().mnr_cc_gram(C.byref(args), _stream()))
  return out


def cc_apply(img, warp, out=None):
  """clip(A(img) @ warp, 0, 1) in float64 (image.py:121-122): img [N,3] float64 on the device, warp [10,3] on the host
  (a sequence or array of floats).  out may be img itself."""
  _chk(img, f64, 'img')
  _chk(out, f64, 'out', allow_none=True)
  N = img.shape[0]
  if img.shape != (N, 3) or (out is not None and out.shape != img.shape):
    raise ValueError(f'cc_apply: img {tuple(img.shape)} (and out) must be [N,3]')
  flat = [float(v) for row in warp for v in row]
  if len(flat) != 3 * L.CC_FEATURES:
    raise ValueError(f'cc_apply: warp must be [10,3], has {len(flat)} values')
  if out is None:
    out = torch.empty_like(img)
  L.check(lib().mnr_cc_apply(N, _ptr(img), (C.c_double * len(flat))(*flat), _ptr(out), _stream()))
  return out


# ----------------------------------------------------------------------------- visualisation (csrc/vis.hip, csrc/camera.hip)


def spherical_rays(camtoworld, height, width):
  """camera_utils.cast_spherical_rays' arrays (camera_utils.py:716-764) for one [3,4] camera: (origins, directions, viewdirs
  [H,W,3], radii [H,W,1], imageplane [H,W,2]), float32 on the device of `camtoworld`."""
  if not _on_device(camtoworld):
    raise ValueError('spherical_rays: camtoworld must be a device tensor (the HIP path has no CPU fallback)')
  c2w = camtoworld[..., :3, :4].to(f32).reshape(3, 4).contiguous()
  H, W = int(height), int(width)
  new = lambda c: torch.empty((H, W, c), dtype=f32, device=c2w.device)
  origins, directions, viewdirs, radii, imageplane = new(3), new(3), new(3), new(1), new(2)
  L.check(lib().mnr_spherical_rays(H, W, _ptr(c2w), _ptr(origins), _ptr(directions), _ptr(viewdirs), _ptr(radii), _ptr(imageplane),
                                   _stream()))
  return origins, directions, viewdirs, radii, imageplane


def camera_record_host(name, record, rows=None):
  """A camera record, or a stack of `rows` of them, as a contiguous float32 host array [.., _lib.CAM_REC] (include/mnerf.h, "The
  forward camera model"; mesh.camera_record builds them), and the one model all of them name.  ValueError for another length,
  values that are not finite, a model that is none of _lib.CAM_MODEL, or models that differ."""
  rec = record.detach().cpu().numpy() if torch.is_tensor(record) else record
  rec = np.ascontiguousarray(rec, dtype=np.float32)
  want = (L.CAM_REC,) if rows is None else (rows, L.CAM_REC)
  if rec.shape != want:
    raise ValueError(f'{name}: the camera record(s) must be {list(want)} float32 (mesh.camera_record), are {list(rec.shape)}')
  if not np.isfinite(rec).all():
    raise ValueError(f'{name}: a camera record holds a value that is not finite')
  models = np.unique(rec.reshape(-1, L.CAM_REC)[:, 25])
  if len(models) > 1 or (len(models) == 1 and float(models[0]) not in (0., 1., 2.)):
    raise ValueError(f'{name}: the records must all name one camera model of {L.CAM_MODEL}, theirs are {models.tolist()}')
  return rec, (int(models[0]) if len(models) else 0)


def project_points(points, record):
  """World points through one camera (mnr_project_points; include/mnerf.h states every operation of the forward model): points
  [n,3] float32 on the device, `record` the _lib.CAM_REC floats of mesh.camera_record (a host array or any tensor) ->
  (uv [n,2] float32, s [n] float32, valid [n] bool).  s is the ray parameter of the point along its pixel's `directions`
  (camera_utils.pixels_to_rays, ops.spherical_rays); valid = in front of the model, inside the fold-back guard and on the image,
  and int(u), int(v) is then the pixel."""
  n = _chk_points('project_points', 'points', points)
  rec, _ = camera_record_host('project_points', record)
  uv = torch.empty((n, 2), dtype=f32, device=points.device)
  s = torch.empty((n,), dtype=f32, device=points.device)
  valid = torch.empty((n,), dtype=torch.uint8, device=points.device)
  L.check(lib().mnr_project_points(n, _ptr(points), rec.ctypes.data_as(C.POINTER(C.c_float)), _ptr(uv), _ptr(s), _ptr(valid), _stream()))
  return uv, s, valid.bool()


def weighted_percentile(x, w, ps, assume_sorted=False, out=None):
  """vis.weighted_percentile (vis.py:22-30): the weighted percentiles `ps` (1 to 4 numbers in [0, 100]) of the values x with
  weights w, both flattened, as a float32 device tensor [len(ps)]; nothing is read back.  The order comes from a stable
  torch.sort; the weight of the i-th sorted value is w[min(order[i], w.numel() - 1)] (a clamping gather, as jax documents)."""
  _chk(x, f32, 'x')
  _chk(w, f32, 'w')
  _chk(out, f32, 'out', allow_none=True)
  ps = [float(p) for p in (ps if hasattr(ps, '__len__') else [ps])]
  if not 1 <= len(ps) <= L.VIS_MAX_PERCENTILES:
    raise ValueError(f'weighted_percentile: {len(ps)} percentiles, 1 to {L.VIS_MAX_PERCENTILES} are taken at once')
  x = x.reshape(-1)
  N, NW = x.numel(), w.numel()
  if assume_sorted:
    xs, order = x, torch.arange(N, dtype=torch.int64, device=x.device)
  else:
    xs, order = torch.sort(x, stable=True)
  partials = torch.empty((max(lib().mnr_weighted_percentile_partials(N), 1),), dtype=f64, device=x.device)
  if out is None:
    out = torch.empty((len(ps),), dtype=f32, device=x.device)
  L.check(lib().mnr_weighted_percentile(N, _ptr(xs), _ptr(order), NW, _ptr(w), len(ps), (C.c_double * len(ps))(*ps), _ptr(partials),
                                        _ptr(out), _stream()))
  return out


def vis_cmap(value, lohi, *, curve=None, modulus=None, lut=None, acc=None, dark=0.8, light=1.0, width=8, out=None, out_u8=None,
             want_f32=True):
  """The per-pixel part of vis.visualize_cmap (vis.py:85-106): value [H,W] or [H,W,1] with a LUT [n,3], [H,W,3] without;
  lohi a float32 device pair (lo, hi) before the curve (None with a modulus); curve None / 'log' / 'neg_log'
  (+-log(x + eps32)) / 'ln' (log(x)); acc [H,W]: matte the result over the checker.  Returns the [H,W,3] float32 image; with out_u8 (a
  [H,W,3] uint8 device tensor) also trunc(clip(., 0, 1) 255) there (want_f32=False: only that, and it is returned)."""
  _chk(value, f32, 'value')
  _chk(lohi, f32, 'lohi', allow_none=True)
  _chk(lut, f32, 'lut', allow_none=True)
  _chk(acc, f32, 'acc', allow_none=True)
  _chk(out, f32, 'out', allow_none=True)
  _chk(out_u8, torch.uint8, 'out_u8', allow_none=True)
  if value.dim() == 2:
    value = value[..., None]
  if value.dim() != 3:
    raise ValueError(f'vis_cmap: value must be [H,W] or [H,W,C], is {tuple(value.shape)}')
  H, W, Cn = (int(v) for v in value.shape)
  if lut is not None and (lut.dim() != 2 or lut.shape[1] != 3):
    raise ValueError(f'vis_cmap: the LUT must be [n,3], is {tuple(lut.shape)}')
  if lohi is not None and lohi.numel() != 2:
    raise ValueError('vis_cmap: lohi must hold two values')
  if acc is not None and tuple(acc.shape) != (H, W):
    raise ValueError(f'vis_cmap: acc {tuple(acc.shape)} must be [{H},{W}]')
  if curve not in L.VIS_CURVE:
    raise ValueError(f'vis_cmap: unknown curve {curve!r}')
  if out is None and (want_f32 or out_u8 is None):
    out = torch.empty((H, W, 3), dtype=f32, device=value.device)
  for o in (out, out_u8):
    if o is not None and tuple(o.shape) != (H, W, 3):
      raise ValueError(f'vis_cmap: an output of shape {tuple(o.shape)} must be [{H},{W},3]')
  a = L.VisCmapArgs()
  a.H, a.W, a.C, a.curve, a.modulus = H, W, Cn, L.VIS_CURVE[curve], float(modulus) if modulus else 0.0
  a.value, a.lohi = value.data_ptr(), None if lohi is None else lohi.data_ptr()
  a.lut, a.n_lut = (None, 0) if lut is None else (lut.data_ptr(), int(lut.shape[0]))
  a.acc, a.dark, a.light, a.width = None if acc is None else acc.data_ptr(), float(dark), float(light), int(width)
  a.out, a.out_u8 = None if out is None else out.data_ptr(), None if out_u8 is None else out_u8.data_ptr()
  L.check(lib().mnr_vis_cmap(C.byref(a), _stream()))
  return out if out is not None else out_u8


def vis_matte(x, acc, *, preop=None, origins=None, directions=None, distance=None, dark=0.8, light=1.0, width=8, out=None):
  """vis.matte (vis.py:39-45) of pre(x) [H,W,C] over the checker with acc [H,W].  preop None, 'half' (x / 2 + 0.5), 'tanh',
  or 'coord_mod' (x is None: ((origins + directions distance + 1) mod 2) / 2, vis.py:109-111,185; without directions and
  distance the origins are the coordinates)."""
  if preop not in L.VIS_PREOP:
    raise ValueError(f'vis_matte: unknown pre-op {preop!r}')
  _chk(acc, f32, 'acc')
  H, W = (int(v) for v in acc.shape)
  a = L.VisMatteArgs()
  if preop == 'coord_mod':
    if (directions is None) != (distance is None):
      raise ValueError('vis_matte: directions and distance go together')
    for t, nm in ((origins, 'origins'), (directions, 'directions')):
      _chk(t, f32, nm, allow_none=nm == 'directions')
      if t is not None and tuple(t.shape) != (H, W, 3):
        raise ValueError(f'vis_matte: {nm} {tuple(t.shape)} must be [{H},{W},3]')
    _chk(distance, f32, 'distance', allow_none=True)
    if distance is not None and tuple(distance.shape) != (H, W):
      raise ValueError(f'vis_matte: distance {tuple(distance.shape)} must be [{H},{W}]')
    Cn = 3
    a.origins = origins.data_ptr()
    if directions is not None:
      a.directions, a.distance = directions.data_ptr(), distance.data_ptr()
  else:
    _chk(x, f32, 'x')
    if x.dim() == 2:
      x = x[..., None]
    if x.dim() != 3 or tuple(x.shape[:2]) != (H, W):
      raise ValueError(f'vis_matte: x {tuple(x.shape)} must be [{H},{W},C]')
    Cn = int(x.shape[2])
    a.x = x.data_ptr()
  _chk(out, f32, 'out', allow_none=True)
  if out is None:
    out = torch.empty((H, W, Cn), dtype=f32, device=acc.device)
  elif tuple(out.shape) != (H, W, Cn):
    raise ValueError(f'vis_matte: out {tuple(out.shape)} must be [{H},{W},{Cn}]')
  a.H, a.W, a.C, a.preop = H, W, Cn, L.VIS_PREOP[preop]
  a.acc, a.dark, a.light, a.width, a.out = acc.data_ptr(), float(dark), float(light), int(width), out.data_ptr()
  L.check(lib().mnr_vis_matte(C.byref(a), _stream()))
  return out


# ----------------------------------------------------------------------------- RawNeRF data path (csrc/raw.hip)


def raw_demosaic(mosaic, black=None, white=None, scale=1.0, n_downsample=1, out=None):
  """raw_utils.load_raw_dataset:354-382 for a stack of RGGB mosaics [N,H,W] (or one [H,W]), uint16 or float32 on the device:
  (raw - black) / (white - black) * scale in float64 (black, white: per-image float64 device tensors [N], or both None),
  bilinear_demosaic in float32, area downsample by n_downsample.  Returns [N, H/n, W/n, 3] ([H/n, W/n, 3]) float32."""
  if mosaic is None or not _on_device(mosaic):
    raise ValueError('raw_demosaic: mosaic must be a device tensor (the HIP path has no CPU fallback)')
  if mosaic.dtype not in (torch.uint16, f32):
    raise ValueError(f'raw_demosaic: mosaic must be uint16 or float32, is {mosaic.dtype}')
  if not mosaic.is_contiguous():
    raise ValueError('raw_demosaic: mosaic must be contiguous')
  single = mosaic.dim() == 2
  if mosaic.dim() not in (2, 3):
    raise ValueError(f'raw_demosaic: mosaic must be [H,W] or [N,H,W], is {tuple(mosaic.shape)}')
  N, H, W = (1,) + tuple(mosaic.shape) if single else tuple(mosaic.shape)
  n = int(n_downsample)
  if (black is None) != (white is None):
    raise ValueError('raw_demosaic: black and white levels go together')
  for t, nm in ((black, 'black'), (white, 'white')):
    _chk(t, f64, nm, allow_none=True)
    if t is not None and t.numel() != N:
      raise ValueError(f'raw_demosaic: {nm} must hold one level per image ({N}), has {t.numel()}')
  _chk(out, f32, 'out', allow_none=True)
  if n < 1 or H % n or W % n:
    raise ValueError(f'raw_demosaic: n_downsample = {n} must divide the image shape [{H}, {W}]')
  shape = (N, H // n, W // n, 3)
  if out is None:
    out = torch.empty(shape, dtype=f32, device=mosaic.device)
  elif out.numel() != N * (H // n) * (W // n) * 3:
    raise ValueError(f'raw_demosaic: out {tuple(out.shape)} must be {shape}')
  if out.data_ptr() % 8:
    raise ValueError('raw_demosaic: out must start at a multiple of 8 bytes (the kernel stores pairs of floats)')
  L.check(lib().mnr_raw_demosaic(N, H, W, L.RAW_DTYPE['float32' if mosaic.dtype == f32 else 'uint16'], _ptr(mosaic), _ptr(black),
                                 _ptr(white), float(scale), n, _ptr(out), _stream()))
  return out.reshape(shape[1:] if single else shape)


def raw_postprocess(raw, camtorgb, exposure=None, *, linear_only=False, want=('f64',)):
  """raw_utils.postprocess_raw in float64 on the device: raw [...,3] float32 or float64, camtorgb nine host floats
  (row-major [3,3]), exposure a host float or a float64 device scalar.  `want`: any of 'f64', 'f32', 'u8'
  (u8 = utils.save_img_u8's truncation); returns the outputs in that order (one tensor when one is asked for).
  linear_only: the float64 raw @ camtorgb.T and nothing else."""
  if raw is None or not _on_device(raw):
    raise ValueError('raw_postprocess: raw must be a device tensor (the HIP path has no CPU fallback)')
  if raw.dtype not in (f32, f64):
    raise ValueError(f'raw_postprocess: raw must be float32 or float64, is {raw.dtype}')
  if raw.shape[-1] != 3:
    raise ValueError(f'raw.shape[-1] is {raw.shape[-1]}, expected 3')
  if not raw.is_contiguous():
    raise ValueError('raw_postprocess: raw must be contiguous')
  m = [float(v) for v in camtorgb]
  if len(m) != 9:
    raise ValueError(f'raw_postprocess: camtorgb must hold 9 values, has {len(m)}')
  want = ('f64',) if linear_only else tuple(want)
  kinds = {'f64': f64, 'f32': f32, 'u8': torch.uint8}
  if not want or any(w not in kinds for w in want):
    raise ValueError(f'raw_postprocess: want {want!r} must name some of {sorted(kinds)}')
  a = L.RawPostArgs()
  a.P, a.raw, a.raw_f64, a.linear_only = raw.numel() // 3, raw.data_ptr(), int(raw.dtype == f64), int(bool(linear_only))
  a.camtorgb = (C.c_double * 9)(*m)
  if isinstance(exposure, torch.Tensor):
    _chk(exposure, f64, 'exposure')
    a.exposure_dev = exposure.data_ptr()
  elif not linear_only:
    if exposure is None:
      raise ValueError('raw_postprocess: needs an exposure')
    a.exposure = float(exposure)
  outs = {w: torch.empty(raw.shape, dtype=kinds[w], device=raw.device) for w in want}
  a.out_f64, a.out_f32, a.out_u8 = (None if w not in outs else outs[w].data_ptr() for w in ('f64', 'f32', 'u8'))
  L.check(lib().mnr_raw_postprocess(C.byref(a), _stream()))
  res = tuple(outs[w] for w in want)
  return res[0] if len(res) == 1 else res


def quantile_f64(x, p, out=None):
  """np.percentile(x, p) of a float64 device tensor (flattened; non-finite values ignored) as a float64 device scalar [1]:
  exact order statistics, numpy's interpolation, no host read."""
  _chk(x, f64, 'x')
  _chk(out, f64, 'out', allow_none=True)
  N = x.numel()
  nbytes = lib().mnr_quantile_f64_workspace(N)
  work = torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=x.device)
  if out is None:
    out = torch.empty((1,), dtype=f64, device=x.device)
  L.check(lib().mnr_quantile_f64(N, _ptr(x), float(p), _ptr(work), _ptr(out), _stream()))
  return out


def affine_sums(est, gt, out=None):
  """The sums behind raw_utils.best_fit_affine(gt, est, axis=(0, 1)): est, gt [...,3] float64 on the device; returns
  [4,3] float64 on the device: per channel the sums of gt, est, gt * est, gt * gt."""
  _chk(est, f64, 'est')
  _chk(gt, f64, 'gt')
  _chk(out, f64, 'out', allow_none=True)
  if est.shape != gt.shape or est.shape[-1] != 3:
    raise ValueError(f'affine_sums: est {tuple(est.shape)} and gt {tuple(gt.shape)} must be two [...,3] images of one shape')
  P = est.numel() // 3
  partials = torch.empty((max(lib().mnr_affine_sums_partials(P), 1),), dtype=f64, device=est.device)
  if out is None:
    out = torch.empty((4, 3), dtype=f64, device=est.device)
  L.check(lib().mnr_affine_sums(P, _ptr(est), _ptr(gt), _ptr(partials), _ptr(out), _stream()))
  return out


def affine_apply(est, a, b, out=None):
  """(est - b) / a per channel: est [...,3] float64 on the device, a and b three host floats each."""
  _chk(est, f64, 'est')
  _chk(out, f64, 'out', allow_none=True)
  if est.shape[-1] != 3 or (out is not None and out.shape != est.shape):
    raise ValueError(f'affine_apply: est {tuple(est.shape)} (and out) must be [...,3]')
  a, b = [float(v) for v in a], [float(v) for v in b]
  if len(a) != 3 or len(b) != 3:
    raise ValueError('affine_apply: a and b must hold three values each')
  if out is None:
    out = torch.empty_like(est)
  L.check(lib().mnr_affine_apply(est.numel() // 3, _ptr(est), (C.c_double * 3)(*a), (C.c_double * 3)(*b), _ptr(out), _stream()))
  return out


def interlevel_loss(mult, t, w, t_env, w_env, stats, g_w_env, *, B_valid):
  for x, nm in ((t, 't'), (w, 'w'), (t_env, 't_env'), (w_env, 'w_env')):
    _chk(x, f32, nm)
  B, n = w.shape
  ne = w_env.shape[1]
  L.check(lib().mnr_interlevel_loss(float(mult), B, B_valid, n, _ptr(t), _ptr(w), ne, _ptr(t_env), _ptr(w_env),
                                    _ptr(stats), _ptr(g_w_env), _stream()))


def distortion_loss(mult, t, w, stats, g_w, *, B_valid):
  _chk(t, f32, 't')
  _chk(w, f32, 'w')
  B, n = w.shape
  L.check(lib().mnr_distortion_loss(float(mult), B, B_valid, n, _ptr(t), _ptr(w), _ptr(stats), _ptr(g_w),
                                    _stream()))


def lossfun_outer(t, w, t_env, w_env):
  for x, nm in ((t, 't'), (w, 'w'), (t_env, 't_env'), (w_env, 'w_env')):
    _chk(x, f32, nm)
  B, n = w.shape
  out = torch.empty((B, n), dtype=f32, device=w.device)
  L.check(lib().mnr_lossfun_outer(B, n, _ptr(t), _ptr(w), w_env.shape[1], _ptr(t_env), _ptr(w_env), _ptr(out),
                                  _stream()))
  return out


def lossfun_distortion(t, w):
  _chk(t, f32, 't')
  _chk(w, f32, 'w')
  B, n = w.shape
  out = torch.empty((B,), dtype=f32, device=w.device)
  L.check(lib().mnr_lossfun_distortion(B, n, _ptr(t), _ptr(w), _ptr(out), _stream()))
  return out


# ----------------------------------------------------------------------------- optimiser


def weight_decay(params, begin, end, mult, grad, loss_out, sqnorm_out=None):
  _chk(params, f32, 'params')
  L.check(lib().mnr_weight_decay(_ptr(params), begin, end, float(mult), _ptr(grad), _ptr(loss_out), _ptr(sqnorm_out),
                                 _stream()))


def grad_sqnorm(grad, begin, end, max_val, out):
  _chk(grad, f32, 'grad')
  _chk(out, f32, 'out')
  L.check(lib().mnr_grad_sqnorm(_ptr(grad), begin, end, float(max_val), _ptr(out), _stream()))


def clip_adam(grad, params, mu, nu, begin, end, sqnorm, *, lr, b1, b2, eps, step, grad_max_val, grad_max_norm):
  for x, nm in ((grad, 'grad'), (params, 'params'), (mu, 'mu'), (nu, 'nu')):
    _chk(x, f32, nm)
  cfg = L.AdamCfg(float(lr), float(b1), float(b2), float(eps), float(1 - b1**step), float(1 - b2**step),
                  float(1 - b1), float(1 - b2), float(grad_max_val), float(grad_max_norm))
  _e = PROFILE.start()
  L.check(lib().mnr_clip_adam(C.byref(cfg), begin, end, _ptr(sqnorm), _ptr(grad), _ptr(params), _ptr(mu),
                              _ptr(nu), _stream()))
  PROFILE.stop(_e, 'clip_adam', 28 * (end - begin))


# ----------------------------------------------------------------------------- image ingest (csrc/ingest.hip)


def image_ingest(src, n_downsample=1, mode='plain', c_out=None, want_alpha=False, out=None, alpha=None):
  """Decoded pixels -> the float32 images a dataset keeps: src [N,H,W,C] (or one [H,W,C]), 1 <= C <= 4, uint8 or float32 on
  the device; the area mean over n_downsample x n_downsample blocks (image.downsample), then by `mode`: 'plain' (`/ 255.` of
  uint8, float32 as it is; the first c_out channels), 'white_bg' (C = 4: `rgb * alpha + (1. - alpha)`, three channels) or
  'normals' (uint8: `x * 2. / 255. - 1.` of the first three channels), in the reference's float32 order (mnr_image_ingest).
  Returns [N,h,w,c_out] float32, and with want_alpha ('white_bg' only) also alpha [N,h,w]."""
  if src is None or not _on_device(src):
    raise ValueError('image_ingest: src must be a device tensor (the HIP path has no CPU fallback)')
  if src.dtype not in (torch.uint8, f32):
    raise ValueError(f'image_ingest: src must be uint8 or float32, is {src.dtype}')
  if not src.is_contiguous():
    raise ValueError('image_ingest: src must be contiguous')
  if src.dim() not in (3, 4):
    raise ValueError(f'image_ingest: src must be [H,W,C] or [N,H,W,C], is {tuple(src.shape)}')
  single = src.dim() == 3
  N, H, W, Cn = ((1,) if single else ()) + tuple(int(v) for v in src.shape)
  if mode not in L.INGEST_MODE:
    raise ValueError(f'image_ingest: mode {mode!r} must be one of {sorted(L.INGEST_MODE)}')
  if not 1 <= Cn <= 4:
    raise ValueError(f'image_ingest: src must have 1 to 4 channels, has {Cn}')
  if c_out is None:
    c_out = Cn if mode == 'plain' else 3
  c_out, n = int(c_out), int(n_downsample)
  if not 1 <= c_out <= Cn:
    raise ValueError(f'image_ingest: c_out = {c_out} must be between 1 and the {Cn} channels of src')
  if n < 1 or H % n or W % n:
    raise ValueError(f'image_ingest: n_downsample = {n} must divide the image shape [{H}, {W}]')
  if src.dtype == torch.uint8 and n > 256:
    raise ValueError(f'image_ingest: n_downsample = {n} > 256 is not available for uint8 input')
  if mode == 'white_bg' and (Cn != 4 or c_out != 3):
    raise ValueError(f'image_ingest: mode \'white_bg\' needs 4 channels in and 3 out, got {Cn} and {c_out}')
  if mode == 'normals' and (src.dtype != torch.uint8 or Cn < 3 or c_out != 3):
    raise ValueError(f'image_ingest: mode \'normals\' needs uint8 input with 3 or 4 channels and c_out = 3')
  if (want_alpha or alpha is not None) and mode != 'white_bg':
    raise ValueError('image_ingest: alpha is an output of mode \'white_bg\' only')
  shape = (N, H // n, W // n, c_out)
  _chk(out, f32, 'out', allow_none=True)
  _chk(alpha, f32, 'alpha', allow_none=True)
  if out is None:
    out = torch.empty(shape, dtype=f32, device=src.device)
  elif out.numel() != N * (H // n) * (W // n) * c_out:
    raise ValueError(f'image_ingest: out {tuple(out.shape)} must be {shape}')
  if alpha is None and want_alpha:
    alpha = torch.empty(shape[:3], dtype=f32, device=src.device)
  elif alpha is not None and alpha.numel() != N * (H // n) * (W // n):
    raise ValueError(f'image_ingest: alpha {tuple(alpha.shape)} must be {shape[:3]}')
  L.check(lib().mnr_image_ingest(N, H, W, Cn, L.IMG_DTYPE['float32' if src.dtype == f32 else 'uint8'], _ptr(src), n,
                                 L.INGEST_MODE[mode], c_out, _ptr(out), _ptr(alpha), _stream()))
  out = out.reshape(shape[1:] if single else shape)
  if alpha is None:
    return out
  return out, alpha.reshape(shape[1:3] if single else shape[:3])


# ----------------------------------------------------------------------------- argument checks the mesh wrappers share


def positive_f32(name, label, x):
  """x as the float32 a kernel sees; ValueError unless that is positive and finite."""
  x = C.c_float(float(x)).value
  if not (x > 0. and math.isfinite(x)):
    raise ValueError(f'{name}: {label} = {x} must be positive and finite in float32')
  return x


def finite3(name, label, v):
  """v (3 numbers or a tensor of 3) as a list of floats; ValueError unless there are three and all are finite."""
  v = [float(x) for x in (v.tolist() if torch.is_tensor(v) else v)]
  if len(v) != 3 or not all(math.isfinite(x) for x in v):
    raise ValueError(f'{name}: {label} must hold 3 finite values, is {v}')
  return v


def _mesh_tensors(name, verts, faces, normals=None, *, max_faces=2 ** 31 - 1, check_index=False):
  """(V, T) of an indexed triangle mesh on the device: `verts` [V,3] float32 (or the vertex count V itself, for an entry that reads
  only the indices), `normals` of the same shape and `faces` [T,3] int32 where given, all contiguous, V below 2^31 and T at most
  `max_faces` (2^31 - 2 where a face id is the low word of a 64-bit key).  check_index makes one min / max read-back and refuses an
  index outside the vertices; without it the kernels skip such a face."""
  if torch.is_tensor(verts):
    _chk(verts, f32, f'{name}: vertices')
    _chk(normals, f32, f'{name}: normals', allow_none=True)
    if verts.dim() != 2 or verts.shape[1] != 3 or (normals is not None and normals.shape != verts.shape):
      raise ValueError(f'{name}: vertices (and normals) must be [V,3], are {tuple(verts.shape)}'
                       + ('' if normals is None else f' and {tuple(normals.shape)}'))
    V = int(verts.shape[0])
  else:
    V = int(verts)
  T = 0
  if faces is not None:
    _chk(faces, torch.int32, f'{name}: faces')
    if faces.dim() != 2 or faces.shape[1] != 3:
      raise ValueError(f'{name}: faces must be [T,3], is {tuple(faces.shape)}')
    T = int(faces.shape[0])
  if not 0 <= V < 2 ** 31 or T > max_faces:
    raise ValueError(f'{name}: {V} vertices and {T} faces: must lie in 0 .. 2^31 - 1 and 0 .. {max_faces}')
  if check_index and T > 0:
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0 or hi >= V:
      raise ValueError(f'{name}: faces holds indices {lo} .. {hi}, outside the {V} vertices')
  return V, T


def check_face_indices(name, faces, n_verts):
  """ValueError if faces [T,3] int32 holds an index outside [0, n_verts): one min / max read-back.  For a caller that launches many
  entries on one mesh and passes them check_faces=False, as mesh.bake_texture does for its chunks."""
  return _mesh_tensors(name, n_verts, faces, check_index=True)


# ----------------------------------------------------------------------------- mesh extraction (csrc/mesh.hip)


def marching_tetrahedra(field, level, origin, spacing, valid=None, return_edges=False):
  """Marching tetrahedra on a regular grid (mnr_mt_classify / mnr_mt_emit_vertices / mnr_mt_emit_faces): field [nx,ny,nz]
  float32 with field[i,j,k] at origin + spacing (i,j,k), inside iff field >= level.  Returns the indexed mesh
  (verts [V,3] float32, normals [V,3] float32, faces [T,3] int32) on the device: vertices ordered by the lower end's linear
  index and edge direction, faces by cell, tetrahedron and triangle, counter-clockwise seen from the low-field side; normals
  point toward lower field.  An isosurface that does not cross the grid gives V = T = 0.  The output sizes depend on the data:
  the per-workgroup counts are scanned with torch.cumsum and the two totals are read back once (the call's one
  synchronisation).

  valid ([nx,ny,nz] bool or uint8 on the device; None: the call, its launches and its results are as above) restricts the mesh
  to observed points: a vertex is kept iff both ends of its grid edge are valid (mnr_mt_vertex_valid, csrc/tsdf.hip), a face
  iff its three vertices are kept, vertices no kept face refers to are removed, and the faces are re-indexed; the order of the
  surviving vertices and faces is unchanged.  (The compaction indexes with boolean masks: one more synchronisation each.)
  return_edges=True appends edges [V,2] int64 to the result: per vertex the linear index of its edge's lower end and the
  edge's direction number 0..6 ((1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1))."""
  if not torch.is_tensor(field) or not _on_device(field):
    raise ValueError('marching_tetrahedra: field must be a device tensor (the HIP path has no CPU fallback)')
  if field.dtype != f32:
    raise ValueError(f'marching_tetrahedra: field must be {f32}, is {field.dtype}')
  if field.dim() != 3 or min(field.shape) < 2:
    raise ValueError(f'marching_tetrahedra: field must be [nx,ny,nz] with every dimension >= 2, is {tuple(field.shape)}')
  if not field.is_contiguous():
    raise ValueError('marching_tetrahedra: field must be contiguous')
  spacing = float(spacing)
  if not (spacing > 0. and math.isfinite(spacing)):
    raise ValueError(f'marching_tetrahedra: spacing must be positive and finite, is {spacing}')
  origin = finite3('marching_tetrahedra', 'origin', origin)
  dev = field.device
  nx, ny, nz = (int(v) for v in field.shape)
  n = nx * ny * nz
  if valid is not None:
    if not torch.is_tensor(valid) or not _on_device(valid) or valid.dtype not in (torch.bool, torch.uint8):
      raise ValueError('marching_tetrahedra: valid must be a bool or uint8 device tensor')
    if tuple(valid.shape) != (nx, ny, nz):
      raise ValueError(f'marching_tetrahedra: valid {tuple(valid.shape)} must have the field\'s shape {(nx, ny, nz)}')
    valid = valid.contiguous().view(torch.uint8)
  nwg = int(lib().mnr_mt_workgroups(n))
  mask = torch.empty((n,), dtype=torch.uint8, device=dev)
  counts = torch.empty((nwg, 2), dtype=torch.int32, device=dev)
  a = L.MtArgs()
  a.nx, a.ny, a.nz, a.field, a.level, a.spacing = nx, ny, nz, field.data_ptr(), float(level), spacing
  a.origin[0], a.origin[1], a.origin[2] = origin
  a.mask, a.counts = mask.data_ptr(), counts.data_ptr()
  L.check(lib().mnr_mt_classify(C.byref(a), _stream()))
  per = counts.t().contiguous()                             # [2, workgroups]: the scan runs along the contiguous dimension
  ends = torch.cumsum(per, 1, dtype=torch.int64)
  offsets = (ends - per).t().contiguous()
  V, T = (int(v) for v in ends[:, -1].tolist())
  if V >= 2 ** 31 or T >= 2 ** 31:
    raise ValueError(f'marching_tetrahedra: {V} vertices and {T} triangles: both must stay below 2^31 (use a coarser grid)')
  verts = torch.empty((V, 3), dtype=f32, device=dev)
  normals = torch.empty((V, 3), dtype=f32, device=dev)
  faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
  if V == 0:
    return (verts, normals, faces) + ((torch.empty((0, 2), dtype=torch.int64, device=dev),) if return_edges else ())
  base = torch.empty((n,), dtype=torch.int32, device=dev)
  a.offsets, a.base = offsets.data_ptr(), base.data_ptr()
  a.verts, a.normals, a.n_verts, a.faces, a.n_faces = verts.data_ptr(), normals.data_ptr(), V, faces.data_ptr(), T
  L.check(lib().mnr_mt_emit_vertices(C.byref(a), _stream()))
  L.check(lib().mnr_mt_emit_faces(C.byref(a), _stream()))
  edges = None
  if return_edges:                                          # vertex order = (lower end, direction) order of the set mask bits
    lower = torch.nonzero(mask).reshape(-1)
    bits = (mask[lower, None] >> torch.arange(7, dtype=torch.uint8, device=dev)) & 1
    at = torch.nonzero(bits)
    edges = torch.stack([lower[at[:, 0]], at[:, 1]], -1)
  if valid is not None:
    keep = torch.empty((V,), dtype=torch.uint8, device=dev)
    L.check(lib().mnr_mt_vertex_valid(C.byref(a), _ptr(valid), _ptr(keep), _stream()))
    keep = keep != 0
    faces = faces[keep[faces.long()].all(-1)]
    used = torch.zeros((V,), dtype=torch.bool, device=dev)
    used[faces.reshape(-1).long()] = True
    new_id = (torch.cumsum(used, 0, dtype=torch.int64) - 1).to(torch.int32)
    faces = new_id[faces.long()].reshape(-1, 3).contiguous()
    verts, normals = verts[used].contiguous(), normals[used].contiguous()
    if edges is not None:
      edges = edges[used].contiguous()
  return (verts, normals, faces) + ((edges,) if return_edges else ())


# ----------------------------------------------------------------------------- TSDF fusion (csrc/tsdf.hip)


def tsdf_integrate(tsdf, weight, color, origin, spacing, trunc, proj, depth, acc=None, rgb=None, acc_threshold=0.5):
  """Fuse F depth images into the running TSDF average of a regular grid, in place (mnr_tsdf_integrate; include/mnerf.h states
  the per-voxel steps): tsdf, weight [nx,ny,nz] float32 and color [nx,ny,nz,3] float32 or None, voxel (i,j,k) at
  origin + spacing (i,j,k); proj [F,3,4] float32 (mesh.world_to_pixel), depth [F,H,W] float32, acc [F,H,W] float32 or None
  (below acc_threshold: an empty ray, the voxel is free space), rgb [F,H,W,3] float32, given iff color is; trunc in world
  units.  A stack longer than _lib.TSDF_MAX_FRAMES is integrated that many frames a launch.  Returns None."""
  name = 'tsdf_integrate'
  for t, label in ((tsdf, 'tsdf'), (weight, 'weight'), (proj, 'proj'), (depth, 'depth')):
    _chk(t, f32, label)
  _chk(color, f32, 'color', allow_none=True)
  _chk(acc, f32, 'acc', allow_none=True)
  _chk(rgb, f32, 'rgb', allow_none=True)
  if tsdf.dim() != 3 or weight.shape != tsdf.shape or (color is not None and tuple(color.shape) != tuple(tsdf.shape) + (3,)):
    raise ValueError(f'{name}: tsdf and weight must be [nx,ny,nz] and color [nx,ny,nz,3]')
  if (color is None) != (rgb is None):
    raise ValueError(f'{name}: rgb and color are both given or both None')
  if depth.dim() != 3 or proj.dim() != 3 or tuple(proj.shape) != (depth.shape[0], 3, 4):
    raise ValueError(f'{name}: depth must be [F,H,W] and proj [F,3,4], are {tuple(depth.shape)} and {tuple(proj.shape)}')
  if (acc is not None and acc.shape != depth.shape) or (rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,)):
    raise ValueError(f'{name}: acc must be [F,H,W] and rgb [F,H,W,3] for depth {tuple(depth.shape)}')
  spacing, trunc = float(spacing), float(trunc)
  if not (spacing > 0. and math.isfinite(spacing)) or not (trunc > 0. and math.isfinite(trunc)):
    raise ValueError(f'{name}: spacing and trunc must be positive and finite, are {spacing} and {trunc}')
  origin = finite3(name, 'origin', origin)
  a = L.TsdfArgs()
  a.nx, a.ny, a.nz = (int(v) for v in tsdf.shape)
  a.origin[0], a.origin[1], a.origin[2] = origin
  a.spacing, a.trunc, a.acc_threshold = spacing, trunc, float(acc_threshold)
  a.F, a.H, a.W = (int(v) for v in depth.shape)
  a.proj, a.depth, a.acc, a.rgb = proj.data_ptr(), depth.data_ptr(), _ptr(acc), _ptr(rgb)
  a.tsdf, a.weight, a.color = tsdf.data_ptr(), weight.data_ptr(), _ptr(color)
  L.check(lib().mnr_tsdf_integrate(C.byref(a), _stream()))


def tsdf_integrate_cam(tsdf, weight, color, origin, spacing, trunc, cameras, depth, acc=None, rgb=None, acc_threshold=0.5):
  """`tsdf_integrate` for any camera model (mnr_tsdf_integrate_cam; include/mnerf.h): instead of proj, cameras [F,_lib.CAM_REC]
  float32 holds one record of mesh.camera_record a frame (a host array or any tensor: it is checked on the host and copied to
  the volumes' device), all of one model and of the images' height and width; depth [F,H,W] holds s, the distance rendered
  along the camera's own rays (the depth of mesh.render_mesh(method='raycast')).  Everything else is tsdf_integrate's."""
  name = 'tsdf_integrate_cam'
  for t, label in ((tsdf, 'tsdf'), (weight, 'weight'), (depth, 'depth')):
    _chk(t, f32, label)
  _chk(color, f32, 'color', allow_none=True)
  _chk(acc, f32, 'acc', allow_none=True)
  _chk(rgb, f32, 'rgb', allow_none=True)
  if tsdf.dim() != 3 or weight.shape != tsdf.shape or (color is not None and tuple(color.shape) != tuple(tsdf.shape) + (3,)):
    raise ValueError(f'{name}: tsdf and weight must be [nx,ny,nz] and color [nx,ny,nz,3]')
  if (color is None) != (rgb is None):
    raise ValueError(f'{name}: rgb and color are both given or both None')
  if depth.dim() != 3:
    raise ValueError(f'{name}: depth must be [F,H,W], is {tuple(depth.shape)}')
  if (acc is not None and acc.shape != depth.shape) or (rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,)):
    raise ValueError(f'{name}: acc must be [F,H,W] and rgb [F,H,W,3] for depth {tuple(depth.shape)}')
  F, H, W = (int(v) for v in depth.shape)
  rec, model = camera_record_host(name, cameras, rows=F)
  if F and not ((rec[:, 26] == H).all() and (rec[:, 27] == W).all()):
    raise ValueError(f'{name}: the records were built for images of another size than depth {tuple(depth.shape)}')
  spacing, trunc = float(spacing), float(trunc)
  if not (spacing > 0. and math.isfinite(spacing)) or not (trunc > 0. and math.isfinite(trunc)):
    raise ValueError(f'{name}: spacing and trunc must be positive and finite, are {spacing} and {trunc}')
  origin = finite3(name, 'origin', origin)
  if F == 0:                                                # (an empty stack has no pointers to hand over)
    return
  rec_dev = torch.from_numpy(rec).to(tsdf.device)
  a = L.TsdfCamArgs()
  a.nx, a.ny, a.nz = (int(v) for v in tsdf.shape)
  a.origin[0], a.origin[1], a.origin[2] = origin
  a.spacing, a.trunc, a.acc_threshold = spacing, trunc, float(acc_threshold)
  a.F, a.H, a.W, a.model = F, H, W, model
  a.cameras, a.depth, a.acc, a.rgb = rec_dev.data_ptr(), depth.data_ptr(), _ptr(acc), _ptr(rgb)
  a.tsdf, a.weight, a.color = tsdf.data_ptr(), weight.data_ptr(), _ptr(color)
  L.check(lib().mnr_tsdf_integrate_cam(C.byref(a), _stream()))


# ----------------------------------------------------------------------------- mesh clean-up (csrc/meshclean.hip)

# sweeps between two read-backs of the convergence flags of `mesh_components`
CC_SWEEPS_PER_READBACK = 4


def mesh_components(faces, n_verts, return_sweeps=False):
  """labels [n_verts] int32 of an indexed triangle mesh (mnr_mesh_cc_init / mnr_mesh_cc_sweep): labels[v] is the smallest vertex
  id v is connected to through face edges, a vertex in no face is its own label.  faces [T,3] int32 on the device; an index
  outside [0, n_verts) raises ValueError (one min / max read-back).  The sweeps run until one of them changes nothing: each
  sweep of a batch of CC_SWEEPS_PER_READBACK has a device flag of its own, and the batch's flags are read back together (the
  loop's one synchronisation per batch); there is no iteration limit.  Integer min only: two runs agree bit for bit.
  return_sweeps=True appends the number of sweeps up to and including the one that changed nothing."""
  V, T = check_face_indices('mesh_components', faces, n_verts)
  labels = torch.empty((V,), dtype=torch.int32, device=faces.device)
  L.check(lib().mnr_mesh_cc_init(V, _ptr(labels), _stream()))
  sweeps = 0
  while V > 0 and T > 0:
    flags = torch.zeros((CC_SWEEPS_PER_READBACK,), dtype=torch.int32, device=faces.device)
    for n in range(CC_SWEEPS_PER_READBACK):
      L.check(lib().mnr_mesh_cc_sweep(_ptr(faces), T, V, _ptr(labels), C.c_void_p(flags.data_ptr() + 4 * n), _stream()))
    flags = flags.tolist()
    if 0 in flags:
      sweeps += flags.index(0) + 1
      break
    sweeps += CC_SWEEPS_PER_READBACK
  return (labels, sweeps) if return_sweeps else labels


def _chk_cell(name, origin, cell):
  return (C.c_float * 3)(*finite3(name, 'origin', origin)), positive_f32(name, 'cell', cell)


def mesh_cluster_keys(verts, origin, cell):
  """keys [V] int64 of the vertices' cells (mnr_mesh_cluster_keys; include/mnerf.h): (cx << 42) | (cy << 21) | cz with
  c = int(floor((x - origin) / cell)) in float32, _lib.MESH_KEY_NONFINITE for a vertex that is not finite, _lib.MESH_KEY_OUTSIDE
  for an index outside [0, 2^21).  No read-back: the caller looks at the smallest key."""
  V, _ = _mesh_tensors('mesh_cluster_keys', verts, None)
  o, cell = _chk_cell('mesh_cluster_keys', origin, cell)
  keys = torch.empty((V,), dtype=torch.int64, device=verts.device)
  L.check(lib().mnr_mesh_cluster_keys(_ptr(verts), V, o, cell, _ptr(keys), _stream()))
  return keys


def mesh_cluster_faces(faces, vmap, n_clusters):
  """(mapped [T,3] int32, canon [T,3] int32, incident [T,3] int32, keep [T] uint8) of the faces under the vertex -> cluster map
  `vmap` [V] int32 (mnr_mesh_cluster_faces): the re-indexed face, the same rotated so that its smallest cluster comes first, each
  cluster the face touches once (-1 in the other slots), and whether its three clusters are distinct."""
  name = 'mesh_cluster_faces'
  _chk(vmap, torch.int32, f'{name}: vmap')
  if vmap.dim() != 1:
    raise ValueError(f'{name}: vmap must be [V], is {tuple(vmap.shape)}')
  V, T = _mesh_tensors(name, vmap.shape[0], faces)
  dev = faces.device
  mapped, canon, incident = (torch.empty((T, 3), dtype=torch.int32, device=dev) for _ in range(3))
  keep = torch.empty((T,), dtype=torch.uint8, device=dev)
  L.check(lib().mnr_mesh_cluster_faces(_ptr(faces), T, _ptr(vmap), V, int(n_clusters), _ptr(mapped), _ptr(canon),
                                       _ptr(incident), _ptr(keep), _stream()))
  return mapped, canon, incident, keep


def mesh_cluster_solve(verts, normals, colors, faces, keys, member_start, members, face_start, cluster_faces, origin, cell):
  """(out_verts [K,3] float32, out_normals [K,3] float32, out_colors [K,3] uint8 or None, fallback [K] uint8) of the K clusters
  (mnr_mesh_cluster_solve; include/mnerf.h states the sums, their order and the closed-form solve): keys [K] int64 the distinct
  cell keys ascending, members [V] int32 with offsets member_start [K+1] int64, cluster_faces [n] int32 with offsets face_start
  [K+1] int64, colors [V,3] uint8 or None.  fallback marks the clusters placed at their centroid."""
  name = 'mesh_cluster_solve'
  V, T = _mesh_tensors(name, verts, faces, normals)
  for t, dt, label in ((keys, torch.int64, 'keys'), (member_start, torch.int64, 'member_start'), (members, torch.int32, 'members'),
                       (face_start, torch.int64, 'face_start'), (cluster_faces, torch.int32, 'cluster_faces')):
    _chk(t, dt, f'{name}: {label}')
  _chk(colors, torch.uint8, f'{name}: colors', allow_none=True)
  K = int(keys.shape[0])
  if colors is not None and colors.shape != verts.shape:
    raise ValueError(f'{name}: colors must be [V,3] like the vertices, is {tuple(colors.shape)}')
  if tuple(member_start.shape) != (K + 1,) or tuple(face_start.shape) != (K + 1,) or tuple(members.shape) != (V,) or cluster_faces.dim() != 1:
    raise ValueError(f'{name}: member_start and face_start must be [K+1], members [V] and cluster_faces a list')
  o, cell = _chk_cell(name, origin, cell)
  dev = verts.device
  out_v = torch.empty((K, 3), dtype=f32, device=dev)
  out_n = torch.empty((K, 3), dtype=f32, device=dev)
  out_c = None if colors is None else torch.empty((K, 3), dtype=torch.uint8, device=dev)
  fallback = torch.empty((K,), dtype=torch.uint8, device=dev)
  a = L.MeshClusterArgs()
  a.n_clusters, a.n_verts, a.n_faces, a.n_incident = K, V, T, int(cluster_faces.shape[0])
  a.verts, a.normals, a.colors, a.faces = verts.data_ptr(), normals.data_ptr(), _ptr(colors), faces.data_ptr()
  a.keys, a.member_start, a.members = keys.data_ptr(), member_start.data_ptr(), members.data_ptr()
  a.face_start, a.cluster_faces = face_start.data_ptr(), cluster_faces.data_ptr()
  a.origin[0], a.origin[1], a.origin[2] = o
  a.cell = cell
  a.out_verts, a.out_normals, a.out_colors, a.fallback = out_v.data_ptr(), out_n.data_ptr(), _ptr(out_c), fallback.data_ptr()
  L.check(lib().mnr_mesh_cluster_solve(C.byref(a), _stream()))
  return out_v, out_n, out_c, fallback


# ----------------------------------------------------------------------------- texture atlas (csrc/atlas.hip)

def atlas_layout(n_faces, cell, cols=None):
  """dict(cell, cols, rows, W, H, n_samples) of the atlas of `n_faces` faces at a cell of `cell` texels (include/mnerf.h): faces
  2k and 2k + 1 share cell k, a cell is (cell + 1) x cell texels, cells fill the atlas row-major `cols` to a row, W = cols (cell + 1),
  rows = ceil(ncells / cols), H = rows cell, n_samples = ncells cell (cell + 1).  The default cols is max(1, ceil(sqrt(ncells cell /
  (cell + 1)))), in integers, which makes the atlas roughly square.  No faces: rows = W = H = n_samples = 0.  Pure Python: the
  one place the layout arithmetic lives on the host."""
  n_faces, cell = int(n_faces), int(cell)
  if cell < L.ATLAS_MIN_CELL:
    raise ValueError(f'atlas_layout: cell = {cell} must be at least {L.ATLAS_MIN_CELL} texels')
  if not 0 <= n_faces < 2 ** 31:
    raise ValueError(f'atlas_layout: {n_faces} faces: must lie in 0 .. 2^31 - 1')
  ncells = (n_faces + 1) // 2
  if cols is None:
    cols = math.isqrt(ncells * cell // (cell + 1))
    while cols * cols * (cell + 1) < ncells * cell:
      cols += 1
    cols = max(1, cols)
  cols = int(cols)
  if cols < 1:
    raise ValueError(f'atlas_layout: cols = {cols} must be at least 1')
  rows = -(-ncells // cols)
  W, H = (cols * (cell + 1) if ncells else 0), rows * cell
  if W >= 2 ** 31 or H >= 2 ** 31:
    raise ValueError(f'atlas_layout: an atlas of {W} x {H} texels: both sides must stay below 2^31')
  return dict(cell=cell, cols=cols, rows=rows, W=W, H=H, n_samples=ncells * cell * (cell + 1))


def _atlas_args(name, m, layout, filter=1.0, check_faces=True):
  """(AtlasArgs, the tensors it points to) of a mesh dict and an `atlas_layout`; face indices outside the vertices raise ValueError
  (one min / max read-back; check_faces=False is for a caller that has made that check on this mesh, as mesh.bake_texture does
  once for all its chunks: the kernels never read outside the vertices, such a face's samples are invalid)."""
  verts, normals, faces = m['vertices'], m['normals'], m['faces']
  V, T = _mesh_tensors(name, verts, faces, normals, check_index=check_faces)
  if layout != atlas_layout(T, layout['cell'], layout['cols']):
    raise ValueError(f'{name}: the layout {layout} is not atlas_layout({T}, {layout["cell"]}, {layout["cols"]})')
  filter = float(filter)
  if not (filter >= 0. and math.isfinite(filter)):
    raise ValueError(f'{name}: filter = {filter} must be finite and not negative')
  a = L.AtlasArgs()
  a.verts, a.normals, a.faces, a.n_verts, a.n_faces = verts.data_ptr(), normals.data_ptr(), faces.data_ptr(), V, T
  a.c, a.cols, a.W, a.H = layout['cell'], layout['cols'], layout['W'], layout['H']
  a.cov_scale = filter * filter / 12.
  return a, (verts, normals, faces)


def _atlas_chunk(name, layout, start, stop):
  start, stop = int(start), int(stop)
  if not 0 <= start <= stop <= layout['n_samples'] or stop - start >= 2 ** 31:
    raise ValueError(f'{name}: samples {start} .. {stop} of {layout["n_samples"]}: a chunk lies inside the atlas and has fewer than 2^31 samples')
  return start, stop - start


def atlas_samples(m, layout, start, stop, filter=1.0, check_faces=True):
  """(means [n,3], covs [n,3,3], normals [n,3], viewdirs [n,3] float32, face [n] int32) of the atlas samples start .. stop - 1 of the
  mesh dict `m` (vertices, normals, faces on the device) under `layout` = atlas_layout(T, cell, cols) (mnr_atlas_samples;
  include/mnerf.h): sample s = cell c (c + 1) + Y (c + 1) + X is a texel, its Gaussian has the texel's position on its face as
  mean and filter^2 / 12 times the second moments of the texel's parallelogram as covariance (filter = 0: a point), its view
  direction is minus the interpolated normal.  face = -1 marks the invalid samples (an odd face count's spare half cell, a face with
  a vertex that is not finite): zero mean and covariance, direction (0, 0, 1)."""
  a, keep = _atlas_args('atlas_samples', m, layout, filter, check_faces)
  s0, n = _atlas_chunk('atlas_samples', layout, start, stop)
  dev = keep[0].device
  means, normals, viewdirs = (torch.empty((n, 3), dtype=f32, device=dev) for _ in range(3))
  covs = torch.empty((n, 3, 3), dtype=f32, device=dev)
  face = torch.empty((n,), dtype=torch.int32, device=dev)
  L.check(lib().mnr_atlas_samples(C.byref(a), s0, n, _ptr(means), _ptr(covs), _ptr(normals), _ptr(viewdirs), _ptr(face), _stream()))
  return means, covs, normals, viewdirs, face


def atlas_store(m, layout, start, rgb, face, atlas, mask, atlas_f32=None, check_faces=True):
  """Write the colours rgb [n,3] float32 of the samples start .. start + n - 1 into atlas [H,W,3] uint8 as floor(clip(rgb, 0, 1) *
  255 + 0.5), set mask [H,W] uint8 to 255 there and, when given, atlas_f32 [H,W,3] float32 to rgb itself (mnr_atlas_store).  face [n]
  int32 is `atlas_samples`' output: samples with face < 0 are skipped.  In place; every texel belongs to one sample."""
  name = 'atlas_store'
  a, keep = _atlas_args(name, m, layout, check_faces=check_faces)
  _chk(rgb, f32, f'{name}: rgb')
  _chk(face, torch.int32, f'{name}: face')
  _chk(atlas, torch.uint8, f'{name}: atlas')
  _chk(mask, torch.uint8, f'{name}: mask')
  _chk(atlas_f32, f32, f'{name}: atlas_f32', allow_none=True)
  n = int(face.shape[0])
  H, W = layout['H'], layout['W']
  if tuple(rgb.shape) != (n, 3) or face.dim() != 1:
    raise ValueError(f'{name}: rgb must be [n,3] and face [n], are {tuple(rgb.shape)} and {tuple(face.shape)}')
  if tuple(atlas.shape) != (H, W, 3) or tuple(mask.shape) != (H, W) or (atlas_f32 is not None and tuple(atlas_f32.shape) != (H, W, 3)):
    raise ValueError(f'{name}: atlas (and atlas_f32) must be [{H},{W},3] and mask [{H},{W}]')
  s0, n = _atlas_chunk(name, layout, start, int(start) + n)
  L.check(lib().mnr_atlas_store(C.byref(a), s0, n, _ptr(rgb), _ptr(face), _ptr(atlas), _ptr(mask), _ptr(atlas_f32), _stream()))


def atlas_uvs(m, layout):
  """uv [T,3,2] float32: (u, v) of the three corners of every face in the atlas of `layout` (mnr_atlas_uvs; include/mnerf.h), the
  inverse of `atlas_samples`' texel -> surface map: u = px / W, v = 1 - py / H with row 0 the top of the image."""
  a, keep = _atlas_args('atlas_uvs', m, layout)
  uv = torch.empty((int(a.n_faces), 3, 2), dtype=f32, device=keep[0].device)
  L.check(lib().mnr_atlas_uvs(C.byref(a), _ptr(uv), _stream()))
  return uv


# ----------------------------------------------------------------------------- mesh rasteriser (csrc/raster.hip)

# box pixels above which a face is rasterised by a workgroup instead of a thread: the A/B of profiles/mesh_render.md
RASTER_THRESHOLD = 128


def _raster_args(name, m, proj, height, width, near, check_index=False):
  """(RasterArgs with the geometry set, the tensors it points to) of a mesh dict (vertices, normals, faces on the device), a [3,4]
  projection (host array or tensor; it is passed by value) and the image size.  Without check_index the kernels skip a face with an
  index outside the vertices."""
  verts, normals, faces = m['vertices'], m['normals'], m['faces']
  V, T = _mesh_tensors(name, verts, faces, normals, max_faces=2 ** 31 - 2, check_index=check_index)
  P = [float(v) for v in torch.as_tensor(proj).detach().cpu().reshape(-1).tolist()]
  if len(P) != 12 or not all(math.isfinite(v) for v in P):
    raise ValueError(f'{name}: proj must be a finite [3,4] matrix')
  height, width, near = int(height), int(width), positive_f32(name, 'near', near)
  if height < 1 or width < 1:
    raise ValueError(f'{name}: an image of {height} x {width} pixels: both sides must be at least 1')
  a = L.RasterArgs()
  a.verts, a.normals, a.faces, a.n_verts, a.n_faces = verts.data_ptr(), normals.data_ptr(), faces.data_ptr(), V, T
  a.proj = (C.c_float * 12)(*P)
  a.H, a.W, a.near = height, width, near
  return a, (verts, normals, faces)


def raster_visibility(m, proj, height, width, near, cull='none', threshold=None, check_faces=True):
  """vis [height,width] int64: the visibility buffer of the mesh dict `m` (vertices, normals, faces on the device) under the [3,4]
  projection `proj` of mesh.world_to_pixel (mnr_raster_visibility; include/mnerf.h states every operation).  A pixel holds the bits
  of the unsigned key (bits(zc) << 32) | face of the nearest face that covers its centre with zc > near (among equal depths the lowest
  id), or all ones (-1) where there is none.  cull = 'back' drops the faces whose geometric normal faces away from the camera.
  `threshold` (default RASTER_THRESHOLD) is the number of bounding-box pixels above which a face is rasterised by a workgroup instead
  of a thread: 0, any value and a huge one give the same buffer bit for bit, as do two runs (integer minimum only).  Face indices
  outside the vertices raise ValueError (one min / max read-back; check_faces=False leaves it to the kernels, which skip such
  a face)."""
  name = 'raster_visibility'
  a, keep = _raster_args(name, m, proj, height, width, near, check_index=check_faces)
  if cull not in L.RASTER_CULL:
    raise ValueError(f"{name}: cull = {cull!r} must be 'none' or 'back'")
  threshold = RASTER_THRESHOLD if threshold is None else int(threshold)
  if not 0 <= threshold < 2 ** 63:
    raise ValueError(f'{name}: threshold = {threshold} must lie in 0 .. 2^63 - 1')
  a.cull, a.threshold = L.RASTER_CULL[cull], threshold
  dev = keep[0].device
  vis = torch.empty((a.H, a.W), dtype=torch.int64, device=dev)
  work = torch.empty((int(a.n_faces) + 1,), dtype=torch.int32, device=dev)        # the large-face list and, last, its counter
  L.check(lib().mnr_raster_visibility(C.byref(a), _ptr(vis), _ptr(work), C.c_void_p(work.data_ptr() + 4 * int(a.n_faces)), _stream()))
  return vis


def _shade_colour_args(name, a, colors, texture, uv, bg):
  """Set the colour source and the background of the RasterArgs `a` (its mesh is set): the checks `raster_shade` and `raycast_shade`
  share."""
  V, T = int(a.n_verts), int(a.n_faces)
  if colors is not None and texture is not None:
    raise ValueError(f'{name}: colors and texture are both given: the colour has one source')
  for t, label, shape in ((colors, 'colors', (V, 3)), (texture, 'texture', None)):
    if t is None:
      continue
    if t.dtype not in (torch.uint8, f32):
      raise ValueError(f'{name}: {label} must be torch.uint8 or torch.float32, is {t.dtype}')
    _chk(t, t.dtype, f'{name}: {label}')
    if (shape is not None and tuple(t.shape) != shape) or (shape is None and (t.dim() != 3 or t.shape[2] != 3 or min(t.shape[:2]) < 1)):
      raise ValueError(f'{name}: {label} must be {"[V,3]" if shape else "a non-empty [Ht,Wt,3] image"}, is {tuple(t.shape)}')
  if texture is not None:
    _chk(uv, f32, f'{name}: uv')
    if tuple(uv.shape) != (T, 3, 2):
      raise ValueError(f'{name}: uv must be [{T},3,2] (three corners a face), is {tuple(uv.shape)}')
    if max(texture.shape[:2]) > 2 ** 24:
      raise ValueError(f'{name}: a texture of {tuple(texture.shape[:2])} texels: a side may not exceed 2^24')
    a.texture, a.texture_u8, a.Ht, a.Wt, a.uv = texture.data_ptr(), int(texture.dtype == torch.uint8), int(texture.shape[0]), int(texture.shape[1]), uv.data_ptr()
  elif uv is not None:
    raise ValueError(f'{name}: uv is given without a texture')
  if colors is not None:
    a.colors, a.colors_u8 = colors.data_ptr(), int(colors.dtype == torch.uint8)
  a.bg = (C.c_float * 3)(*finite3(name, 'bg', bg))


def raster_shade(m, proj, vis, near, colors=None, texture=None, uv=None, bg=(1., 1., 1.)):
  """dict(face [H,W] int32, depth [H,W], acc [H,W], bary [H,W,3], normals [H,W,3], rgb [H,W,3] float32) of a visibility buffer `vis`
  [H,W] int64 that `raster_visibility` wrote for the same mesh, projection and near (mnr_raster_shade; include/mnerf.h): the winning
  face (-1: none), its zc, 1 where there is one, the perspective-correct barycentrics, the interpolated unit normal and the colour:
  `colors` [V,3] uint8 or float32 blended over the face, or `texture` [Ht,Wt,3] uint8 or float32 looked up bilinearly at the blend of
  `uv` [T,3,2] (per face corner, v = 1 the top row: what mesh.bake_texture returns), or, with neither, 0.5 + 0.5 normal.  Pixels
  without a face get `bg`."""
  name = 'raster_shade'
  _chk(vis, torch.int64, f'{name}: vis')
  if vis.dim() != 2:
    raise ValueError(f'{name}: vis must be [H,W], is {tuple(vis.shape)}')
  H, W = int(vis.shape[0]), int(vis.shape[1])
  a, keep = _raster_args(name, m, proj, H, W, near)
  _shade_colour_args(name, a, colors, texture, uv, bg)
  dev = vis.device
  out = dict(face=torch.empty((H, W), dtype=torch.int32, device=dev), depth=torch.empty((H, W), dtype=f32, device=dev),
             acc=torch.empty((H, W), dtype=f32, device=dev), bary=torch.empty((H, W, 3), dtype=f32, device=dev),
             normals=torch.empty((H, W, 3), dtype=f32, device=dev), rgb=torch.empty((H, W, 3), dtype=f32, device=dev))
  L.check(lib().mnr_raster_shade(C.byref(a), _ptr(vis), _ptr(out['face']), _ptr(out['depth']), _ptr(out['acc']), _ptr(out['bary']),
                                 _ptr(out['normals']), _ptr(out['rgb']), _stream()))
  return out


# ----------------------------------------------------------------------------- view-dependent texture (csrc/shtex.hip)


def _sh_degree(name, degree):
  if isinstance(degree, bool) or int(degree) != degree or not 0 <= int(degree) <= L.SHTEX_MAX_DEGREE:
    raise ValueError(f'{name}: degree = {degree!r} must be an integer in 0 .. {L.SHTEX_MAX_DEGREE}')
  return int(degree)


def sh_basis(dirs, degree):
  """Y [D,K] float64 (NumPy), K = (degree + 1)^2: the real spherical harmonics of include/mnerf.h at the directions `dirs` [D,3]
  (a host array or a tensor; they are rounded to float32 first, what the kernels see, and evaluated in float64): the constant, then
  y, z, x, then xy, yz, 3z^2 - 1, xz, x^2 - y^2, each with its constant.  The directions are taken as they are (unit vectors are
  the caller's business)."""
  import numpy as np
  degree = _sh_degree('sh_basis', degree)
  d = np.asarray(dirs.detach().cpu().numpy() if torch.is_tensor(dirs) else dirs, dtype=np.float32).astype(np.float64)
  if d.ndim != 2 or d.shape[1] != 3:
    raise ValueError(f'sh_basis: dirs must be [D,3], is {d.shape}')
  x, y, z = d[:, 0], d[:, 1], d[:, 2]
  c0, c1, c2a, c2b, c2c = L.SH_CONSTANTS
  cols = [np.full_like(x, c0)]
  if degree >= 1:
    cols += [c1 * y, c1 * z, c1 * x]
  if degree >= 2:
    cols += [c2a * (x * y), c2a * (y * z), c2b * (3. * (z * z) - 1.), c2a * (x * z), c2c * (x * x - y * y)]
  return np.ascontiguousarray(np.stack(cols, -1))


def _shtex_dirs(name, dirs, normals):
  _chk(dirs, f32, f'{name}: dirs')
  _chk(normals, f32, f'{name}: normals')
  if dirs.dim() != 2 or dirs.shape[1] != 3 or not 1 <= dirs.shape[0] <= L.SHTEX_MAX_DIRS:
    raise ValueError(f'{name}: dirs must be [D,3] with D in 1 .. {L.SHTEX_MAX_DIRS}, is {tuple(dirs.shape)}')
  if normals.dim() != 2 or normals.shape[1] != 3 or normals.shape[0] >= 2 ** 31:
    raise ValueError(f'{name}: normals must be [n,3] with n below 2^31, is {tuple(normals.shape)}')
  return int(dirs.shape[0]), int(normals.shape[0])


def shtex_weights(dirs, normals):
  """w [n,D] float32: the weight min(max(-dot(d_k, n), 0), 1) of every direction of `dirs` [D,3] for every unit normal of `normals`
  [n,3] (mnr_shtex_weights; include/mnerf.h).  A view direction points from the eye to the surface, so w > 0 marks the directions
  a texel can be seen from; NaN gives 0."""
  D, n = _shtex_dirs('shtex_weights', dirs, normals)
  w = torch.empty((n, D), dtype=f32, device=normals.device)
  L.check(lib().mnr_shtex_weights(_ptr(dirs), D, _ptr(normals), n, _ptr(w), _stream()))
  return w


def shtex_fit(dirs, normals, rgb, degree, lam=0., basis=None):
  """coef [n,K,3] float32, K = (degree + 1)^2: per texel the spherical-harmonic coefficients that fit the colours rgb [n,D,3] float32
  of the directions `dirs` [D,3] in weighted ridge least squares, weights as in `shtex_weights` for the texel's `normals` [n,3]
  (mnr_shtex_fit; include/mnerf.h states every operation: float64 normal equations, Cholesky, one rounding to float32).  A direction
  with weight 0 is not read; one whose colour is not finite is skipped.  `lam` >= 0 is the ridge relative to the mean diagonal
  entry, on all coefficients but the constant.  A texel whose system cannot be solved gets its weighted mean colour as a constant,
  one without any usable direction zeros; every output is finite.  `basis` is `sh_basis(dirs, degree)` on the device (float64
  [D,K]) for a caller that fits many chunks; by default it is computed here."""
  name = 'shtex_fit'
  D, n = _shtex_dirs(name, dirs, normals)
  degree = _sh_degree(name, degree)
  K = (degree + 1) ** 2
  lam = float(lam)
  if not (lam >= 0. and math.isfinite(lam)):
    raise ValueError(f'{name}: lam = {lam} must be finite and not negative')
  _chk(rgb, f32, f'{name}: rgb')
  if tuple(rgb.shape) != (n, D, 3):
    raise ValueError(f'{name}: rgb must be [{n},{D},3], is {tuple(rgb.shape)}')
  if basis is None:
    basis = torch.from_numpy(sh_basis(dirs, degree)).to(normals.device)
  _chk(basis, torch.float64, f'{name}: basis')
  if tuple(basis.shape) != (D, K):
    raise ValueError(f'{name}: basis must be [{D},{K}], is {tuple(basis.shape)}')
  coef = torch.empty((n, K, 3), dtype=f32, device=normals.device)
  L.check(lib().mnr_shtex_fit(_ptr(dirs), _ptr(basis), D, degree, _ptr(normals), _ptr(rgb), n, lam, _ptr(coef), _stream()))
  return coef


def shtex_shade(m, face, bary, uv, sh, origin, rgb):
  """Overwrite rgb [H,W,3] float32, in place, with the view-dependent colour of every pixel that shows a face (mnr_shtex_shade;
  include/mnerf.h): `face` [H,W] int32 and `bary` [H,W,3] float32 are `raster_shade`'s outputs for the mesh dict `m`, `uv` [T,3,2] and
  `sh` [Ht,Wt,K,3] float32 (K = 1, 4 or 9 sets the degree) the atlas of mesh.bake_texture(..., sh_degree=), `origin` the eye.  The
  view direction is the unit vector from the eye to the pixel's surface point; every coefficient plane is looked up bilinearly like
  a texture, the sum over the basis is clipped to [0, 1].  Pixels with face < 0 keep what rgb holds.  Returns rgb."""
  name = 'shtex_shade'
  verts, faces = m['vertices'], m['faces']
  V, T = _mesh_tensors(name, verts, faces, max_faces=2 ** 31 - 2)
  _chk(face, torch.int32, f'{name}: face')
  _chk(bary, f32, f'{name}: bary')
  _chk(uv, f32, f'{name}: uv')
  _chk(sh, f32, f'{name}: sh')
  _chk(rgb, f32, f'{name}: rgb')
  if face.dim() != 2 or min(face.shape) < 1 or tuple(bary.shape) != tuple(face.shape) + (3,) or tuple(rgb.shape) != tuple(bary.shape):
    raise ValueError(f'{name}: face must be a non-empty [H,W] and bary and rgb [H,W,3], are {tuple(face.shape)}, {tuple(bary.shape)} and {tuple(rgb.shape)}')
  if tuple(uv.shape) != (T, 3, 2):
    raise ValueError(f'{name}: uv must be [{T},3,2] (three corners a face), is {tuple(uv.shape)}')
  degrees = {(d + 1) ** 2: d for d in range(L.SHTEX_MAX_DEGREE + 1)}
  if sh.dim() != 4 or sh.shape[3] != 3 or sh.shape[2] not in degrees or min(sh.shape[:2]) < 1 or max(sh.shape[:2]) > 2 ** 24:
    raise ValueError(f'{name}: sh must be [Ht,Wt,K,3] with K in {sorted(degrees)} and 1 .. 2^24 texels a side, is {tuple(sh.shape)}')
  a = L.ShtexShadeArgs()
  a.verts, a.faces, a.n_verts, a.n_faces = verts.data_ptr(), faces.data_ptr(), V, T
  a.face, a.bary, a.H, a.W = face.data_ptr(), bary.data_ptr(), int(face.shape[0]), int(face.shape[1])
  a.uv, a.sh, a.Ht, a.Wt, a.degree = uv.data_ptr(), sh.data_ptr(), int(sh.shape[0]), int(sh.shape[1]), degrees[int(sh.shape[2])]
  a.origin = (C.c_float * 3)(*finite3(name, 'origin', origin))
  L.check(lib().mnr_shtex_shade(C.byref(a), _ptr(rgb), _stream()))
  return rgb


# ----------------------------------------------------------------------------- mesh geometry (csrc/meshdist.hip)

# `mesh_grid_build` coarsens its cell (times 2) while the grid holds more than this many (cell, face) pairs a valid face
MESH_GRID_PAIRS_PER_FACE = 8


def _chk_mesh(name, verts, faces, check_index=False):
  return _mesh_tensors(name, verts, faces, max_faces=2 ** 31 - 2, check_index=check_index)


def mesh_face_areas(verts, faces):
  """area [T] float64 of the faces (mnr_mesh_face_areas; include/mnerf.h): 0.5 |(b - a) x (c - a)| in float64 from the float32
  corners, 0 for a face with an index outside the vertices or a corner that is not finite."""
  V, T = _chk_mesh('mesh_face_areas', verts, faces)
  area = torch.empty((T,), dtype=torch.float64, device=verts.device)
  L.check(lib().mnr_mesh_face_areas(_ptr(verts), V, _ptr(faces), T, _ptr(area), _stream()))
  return area


def mesh_sample(verts, faces, cum, n, seed):
  """(points [n,3] float32, face [n] int32): n points on the surface, stratified in the area (mnr_mesh_sample; include/mnerf.h).  `cum`
  [T] float64 is the inclusive running sum of `mesh_face_areas` (the caller's: the order of that sum is not part of the contract);
  sample i lands on the first face whose cum exceeds (i + 0.5) / n of the total, at barycentrics from a 32-bit integer mix of
  (seed, i).  The total must be positive and finite (one read-back)."""
  name = 'mesh_sample'
  V, T = _chk_mesh(name, verts, faces)
  _chk(cum, torch.float64, f'{name}: cum')
  if tuple(cum.shape) != (T,):
    raise ValueError(f'{name}: cum must be [{T}], is {tuple(cum.shape)}')
  n, seed = int(n), int(seed)
  if not 0 <= n < 2 ** 31:
    raise ValueError(f'{name}: n = {n} must lie in 0 .. 2^31 - 1')
  if not 0 <= seed < 2 ** 32:
    raise ValueError(f'{name}: seed = {seed} must lie in 0 .. 2^32 - 1')
  points = torch.empty((n, 3), dtype=f32, device=verts.device)
  face = torch.empty((n,), dtype=torch.int32, device=verts.device)
  if n == 0:
    return points, face
  total = float(cum[-1]) if T > 0 else 0.
  if not (total > 0. and math.isfinite(total)):
    raise ValueError(f'{name}: the total area is {total}: there is no surface to sample')
  L.check(lib().mnr_mesh_sample(_ptr(verts), V, _ptr(faces), T, _ptr(cum), n, seed, _ptr(points), _ptr(face), _stream()))
  return points, face


def _meshdist_args(verts, faces, origin, hi, cell, dims):
  a = L.MeshDistArgs()
  a.verts, a.faces, a.n_verts, a.n_faces = verts.data_ptr(), faces.data_ptr(), int(verts.shape[0]), int(faces.shape[0])
  a.origin, a.hi, a.cell, a.dims = (C.c_float * 3)(*origin), (C.c_float * 3)(*hi), cell, (C.c_int * 3)(*dims)
  return a


def _grid_dims(origin, hi, cell):
  """dims_a = cell(hi_a) + 1 with the kernels' float32 arithmetic (include/mnerf.h)."""
  import numpy as np
  o, h = np.asarray(origin, dtype=np.float32), np.asarray(hi, dtype=np.float32)
  return [int(v) + 1 for v in np.floor((h - o) / np.float32(cell))]


def mesh_grid_build(verts, faces, cell=None):
  """A uniform grid over the faces for `point_mesh_distance` (mnr_mesh_grid_count / mnr_mesh_grid_fill; include/mnerf.h): a dict of
  origin and hi (3 floats each: the box of the corners of the valid faces), cell, dims (3 ints), cell_start [cells + 1] int64 and
  pair_faces [pairs] int32 (cell (x, y, z), linear index (x dims[1] + y) dims[2] + z, holds pair_faces[cell_start[i] :
  cell_start[i + 1]], ascending), n_valid and pairs.  A face is registered in every cell its axis-aligned box overlaps.

  The cell, when not given (a decision, not a derived number): with e_1 >= e_2 >= e_3 the box's extents and T the number of valid
  faces, the largest of e_1 / T, sqrt(e_1 e_2 / T) and cbrt(e_1 e_2 e_3 / T), so that the grid has about as many cells as there are
  faces whether the box is a volume, a slab or a line (1 if all three vanish), and at least e_1 / (MAX_DIM - 1), MAX_DIM = 1024
  cells an axis being the kernels' limit.  Then the pairs are counted (one read-back) and the cell is doubled, and the count repeated,
  while they exceed MESH_GRID_PAIRS_PER_FACE = 8 a valid face: a few faces that span the scene must not blow the list up, and a single
  cell ends it at one pair a face.  A given `cell` is taken as it is (ValueError if it needs more than MAX_DIM cells an axis).
  The scan, the stable sort by cell and cell_start (bincount, cumsum) are torch on the device; the pair list is the same in every
  run.  No valid face: a grid of one empty cell."""
  name = 'mesh_grid_build'
  V, T = _chk_mesh(name, verts, faces)
  dev = verts.device
  if cell is not None:
    cell = positive_f32(name, 'cell', cell)
  empty = dict(origin=[0., 0., 0.], hi=[0., 0., 0.], cell=1. if cell is None else cell, dims=[1, 1, 1], n_valid=0, pairs=0,
               cell_start=torch.zeros((2,), dtype=torch.int64, device=dev), pair_faces=torch.zeros((0,), dtype=torch.int32, device=dev))
  if T == 0 or V == 0:
    return empty
  idx = faces.long()
  ok = ((idx >= 0) & (idx < V)).all(1)
  corners = verts[idx.clamp(0, V - 1)]
  ok &= torch.isfinite(corners).all(2).all(1)
  n_valid = int(ok.sum())
  if n_valid == 0:
    return empty
  corners = corners[ok].reshape(-1, 3)
  origin, hi = corners.min(0).values.tolist(), corners.max(0).values.tolist()
  del corners, idx
  forced = cell is not None
  if not forced:
    e = sorted((h - o for o, h in zip(origin, hi)), reverse=True)
    cell = max(e[0] / n_valid, math.sqrt(e[0] * e[1] / n_valid), (e[0] * e[1] * e[2] / n_valid) ** (1. / 3.), e[0] / (L.MESHDIST_MAX_DIM - 1))
    cell = C.c_float(cell if cell > 0. else 1.).value
  while True:
    dims = _grid_dims(origin, hi, cell)
    if max(dims) > L.MESHDIST_MAX_DIM:
      if forced:
        raise ValueError(f'{name}: cell = {cell:.6g} needs {dims} cells: at most {L.MESHDIST_MAX_DIM} an axis')
      cell = C.c_float(2. * cell).value                      # (rounding of the automatic cell at the limit)
      continue
    a = _meshdist_args(verts, faces, origin, hi, cell, dims)
    counts = torch.empty((T,), dtype=torch.int64, device=dev)
    L.check(lib().mnr_mesh_grid_count(C.byref(a), _ptr(counts), _stream()))
    offsets = torch.cat([torch.zeros((1,), dtype=torch.int64, device=dev), torch.cumsum(counts, 0)])
    pairs = int(offsets[-1])
    if forced or pairs <= MESH_GRID_PAIRS_PER_FACE * n_valid:
      break
    cell = C.c_float(2. * cell).value
  if pairs >= 2 ** 31:
    raise ValueError(f'{name}: cell = {cell:.6g} gives {pairs} (cell, face) pairs: must stay below 2^31')
  pair_cell = torch.empty((pairs,), dtype=torch.int32, device=dev)
  pair_face = torch.empty((pairs,), dtype=torch.int32, device=dev)
  L.check(lib().mnr_mesh_grid_fill(C.byref(a), _ptr(offsets), pairs, _ptr(pair_cell), _ptr(pair_face), _stream()))
  cells = dims[0] * dims[1] * dims[2]
  pair_cell = pair_cell.long()
  by_cell = torch.sort(pair_cell, stable=True).indices       # face-major list: a cell's faces stay ascending
  cell_start = torch.cat([torch.zeros((1,), dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(pair_cell, minlength=cells), 0)])
  return dict(origin=origin, hi=hi, cell=cell, dims=dims, n_valid=n_valid, pairs=pairs, cell_start=cell_start.contiguous(),
              pair_faces=pair_face[by_cell].contiguous())


def point_mesh_distance(points, verts, faces, max_dist=None, grid=None, cell=None, check_faces=True, return_shells=False):
  """(d2 [N] float32, face [N] int32): the squared distance of every point to the nearest face of the mesh and the lowest id of a
  face that attains it (mnr_mesh_distance; include/mnerf.h states the formula, every operation in its order).  A point cloud is a
  mesh whose faces are (i, i, i).  With `max_dist` (positive, finite) only faces with d2 <= max_dist^2 (float32) count.  Where no
  face counts, or the point is not finite: d2 = +inf, face = -1.  The result is a minimum of (bits(d2) << 32 | face) keys over a set
  of faces: it does not depend on the grid or the order of traversal; two runs, and two grids, agree bit for bit.

  `grid` is a `mesh_grid_build` result for the same verts and faces (built here when None, with `cell` as its override).  The
  queries are sorted by their cell (torch) so that the lanes of a wave walk the same cells; the results come back in the caller's
  order.  Face indices outside the vertices raise ValueError (one min / max read-back; check_faces=False leaves it to the kernels,
  which skip such a face, as they skip one with a corner that is not finite).  N = 0 or no valid face launches nothing.
  return_shells=True appends shells [N] int32, the Chebyshev shells of cells each query visited."""
  name = 'point_mesh_distance'
  _chk(points, f32, f'{name}: points')
  if points.dim() != 2 or points.shape[1] != 3:
    raise ValueError(f'{name}: points must be [N,3], is {tuple(points.shape)}')
  V, T = _chk_mesh(name, verts, faces, check_index=check_faces)
  lim = float('inf') if max_dist is None else positive_f32(name, 'max_dist', max_dist)
  if grid is not None and cell is not None:
    raise ValueError(f'{name}: grid and cell are both given')
  N, dev = int(points.shape[0]), points.device
  d2 = torch.full((N,), float('inf'), dtype=f32, device=dev)
  face = torch.full((N,), -1, dtype=torch.int32, device=dev)
  shells = torch.zeros((N,), dtype=torch.int32, device=dev) if return_shells else None
  out = (d2, face, shells) if return_shells else (d2, face)
  if N == 0 or T == 0 or V == 0:
    return out
  if grid is None:
    grid = mesh_grid_build(verts, faces, cell=cell)
  cell_start, pair_faces, dims = grid['cell_start'], grid['pair_faces'], [int(v) for v in grid['dims']]
  _chk(cell_start, torch.int64, f'{name}: grid cell_start')
  _chk(pair_faces, torch.int32, f'{name}: grid pair_faces')
  if len(dims) != 3 or min(dims) < 1 or tuple(cell_start.shape) != (dims[0] * dims[1] * dims[2] + 1,) or pair_faces.dim() != 1:
    raise ValueError(f'{name}: grid: cell_start must be [{dims} cells + 1] and pair_faces a list')
  P = int(pair_faces.shape[0])
  if P == 0:
    return out
  origin, hi = [float(v) for v in grid['origin']], [float(v) for v in grid['hi']]
  a = _meshdist_args(verts, faces, origin, hi, C.c_float(float(grid['cell'])).value, dims)
  o, h = torch.tensor(origin, dtype=f32, device=dev), torch.tensor(hi, dtype=f32, device=dev)
  g = torch.nan_to_num(((torch.minimum(torch.maximum(points, o), h) - o) / a.cell).floor(), nan=0.)
  g = torch.minimum(g.clamp(min=0.), torch.tensor([d - 1 for d in dims], dtype=f32, device=dev)).long()
  order = torch.sort((g[:, 0] * dims[1] + g[:, 1]) * dims[2] + g[:, 2]).indices.contiguous()
  L.check(lib().mnr_mesh_distance(C.byref(a), _ptr(cell_start), _ptr(pair_faces), P, _ptr(points), _ptr(order), N, lim, _ptr(d2), _ptr(face),
                                  _ptr(shells), _stream()))
  return out


# ----------------------------------------------------------------------------- mesh ray casting (csrc/meshray.hip)

RAY_TILE = 8                       # an 8 x 8 pixel tile is one wave of mnr_mesh_raycast


def pixel_tile_order(height, width, device):
  """order [height width] int64 for `mesh_raycast`: the row-major pixel indices of an image, tile by tile (RAY_TILE x RAY_TILE pixels,
  row-major inside a tile), so that a wave of 64 threads serves one tile and its lanes walk the same cells."""
  ys, xs = torch.meshgrid(torch.arange(int(height), device=device), torch.arange(int(width), device=device), indexing='ij')
  tiles_x = (int(width) + RAY_TILE - 1) // RAY_TILE
  key = ((ys // RAY_TILE) * tiles_x + xs // RAY_TILE) * (RAY_TILE * RAY_TILE) + (ys % RAY_TILE) * RAY_TILE + xs % RAY_TILE
  return torch.sort(key.reshape(-1)).indices.contiguous()


def _grid_tensors(name, grid, T, check_faces):
  """(cell_start, pair_faces, dims, pairs) of a `mesh_grid_build` result, checked against each other and, with check_faces, against
  the T faces of the mesh it is used with (one max read-back)."""
  cell_start, pair_faces, dims = grid['cell_start'], grid['pair_faces'], [int(v) for v in grid['dims']]
  _chk(cell_start, torch.int64, f'{name}: grid cell_start')
  _chk(pair_faces, torch.int32, f'{name}: grid pair_faces')
  if len(dims) != 3 or min(dims) < 1 or tuple(cell_start.shape) != (dims[0] * dims[1] * dims[2] + 1,) or pair_faces.dim() != 1:
    raise ValueError(f'{name}: grid: cell_start must be [{dims} cells + 1] and pair_faces a list')
  P = int(pair_faces.shape[0])
  if check_faces and P > 0 and int(pair_faces.max()) >= T:
    raise ValueError(f'{name}: grid: pair_faces names face {int(pair_faces.max())} of a mesh of {T} faces: the grid was built for another mesh')
  return cell_start, pair_faces, dims, P


def mesh_raycast(origins, directions, verts, faces, t_min=0., t_max=None, cull='none', grid=None, cell=None, order=None, check_faces=True):
  """(t [N] float32, face [N] int32, bary [N,3] float32): the nearest intersection of every ray origins[i] + t directions[i] ([N,3]
  float32 each; the directions are NOT normalised, t is in units of their length) with the mesh (mnr_mesh_raycast; include/mnerf.h
  states the watertight hit test, every operation in its order): the smallest t in (t_min, t_max], the lowest id among the faces that
  attain it and the barycentrics of the hit on that face.  t_max=None: no upper limit.  cull = 'back' counts only faces whose corners
  run counter-clockwise seen from the ray origin (the rasteriser's front).  Where nothing is hit, or the ray is not finite or has no
  direction: t = +inf, face = -1, bary = 0.  The result is a minimum of (bits(t) << 32 | face) keys over the faces that pass a test
  which does not know the grid: it does not depend on the grid, on `order` or on the order of the rays; two runs agree bit for bit.

  `grid` is a `mesh_grid_build` result for the same verts and faces (built here when None, with `cell` as its override).  `order` [N]
  int64 is a permutation of the rays: thread i serves ray order[i] (`pixel_tile_order` for the rays of an image); None sorts the
  rays by the cell in which they enter the grid's box (torch), so that the lanes of a wave walk the same cells.  Face indices outside
  the vertices raise ValueError (check_faces=False leaves them to the kernel, which skips such a face).  N = 0, no face or an empty
  grid launches nothing."""
  name = 'mesh_raycast'
  _chk(origins, f32, f'{name}: origins')
  _chk(directions, f32, f'{name}: directions')
  if origins.dim() != 2 or origins.shape[1] != 3 or tuple(directions.shape) != tuple(origins.shape):
    raise ValueError(f'{name}: origins and directions must be [N,3], are {tuple(origins.shape)} and {tuple(directions.shape)}')
  V, T = _chk_mesh(name, verts, faces, check_index=check_faces)
  t_min = C.c_float(float(t_min)).value
  t_max = float('inf') if t_max is None else C.c_float(float(t_max)).value
  if not (t_min >= 0. and math.isfinite(t_min)):
    raise ValueError(f'{name}: t_min = {t_min} must be finite and not negative')
  if not t_max > t_min:
    raise ValueError(f'{name}: t_max = {t_max} must exceed t_min = {t_min}')
  if cull not in L.RASTER_CULL:
    raise ValueError(f"{name}: cull = {cull!r} must be 'none' or 'back'")
  if grid is not None and cell is not None:
    raise ValueError(f'{name}: grid and cell are both given')
  N, dev = int(origins.shape[0]), origins.device
  if order is not None:
    _chk(order, torch.int64, f'{name}: order')
    if tuple(order.shape) != (N,):
      raise ValueError(f'{name}: order must be [{N}], is {tuple(order.shape)}')
  t = torch.full((N,), float('inf'), dtype=f32, device=dev)
  face = torch.full((N,), -1, dtype=torch.int32, device=dev)
  bary = torch.zeros((N, 3), dtype=f32, device=dev)
  if N == 0 or T == 0 or V == 0:
    return t, face, bary
  if grid is None:
    grid = mesh_grid_build(verts, faces, cell=cell)
  cell_start, pair_faces, dims, P = _grid_tensors(name, grid, T, check_faces)
  if P == 0:
    return t, face, bary
  lo, hi = [float(v) for v in grid['origin']], [float(v) for v in grid['hi']]
  a = _meshdist_args(verts, faces, lo, hi, C.c_float(float(grid['cell'])).value, dims)
  if order is None:                                          # by the cell of the point where the ray enters the box (an ordering only)
    o, h = torch.tensor(lo, dtype=f32, device=dev), torch.tensor(hi, dtype=f32, device=dev)
    inv = 1. / directions
    near = torch.minimum((o - origins) * inv, (h - origins) * inv)
    enter = torch.nan_to_num(near, nan=-float('inf')).max(1).values.clamp(min=t_min, max=3e38)
    p = torch.nan_to_num(origins + enter[:, None] * directions, nan=0., posinf=3e38, neginf=-3e38)
    g = ((torch.minimum(torch.maximum(p, o), h) - o) / a.cell).floor()
    g = torch.minimum(g.clamp(min=0.), torch.tensor([d - 1 for d in dims], dtype=f32, device=dev)).long()
    order = torch.sort((g[:, 0] * dims[1] + g[:, 1]) * dims[2] + g[:, 2]).indices.contiguous()
  L.check(lib().mnr_mesh_raycast(C.byref(a), _ptr(cell_start), _ptr(pair_faces), P, _ptr(origins), _ptr(directions), _ptr(order), N, t_min, t_max,
                                 L.RASTER_CULL[cull], _ptr(t), _ptr(face), _ptr(bary), _stream()))
  return t, face, bary


def raycast_shade(m, face, bary, colors=None, texture=None, uv=None, bg=(1., 1., 1.)):
  """dict(normals [..,3], rgb [..,3] float32) of the hits `face` [..] int32 and `bary` [..,3] float32 that `mesh_raycast` returned for
  the mesh dict `m` (vertices, normals, faces on the device), in their leading shape (mnr_raycast_shade; include/mnerf.h): the colour
  and normal stage of `raster_shade`, the same operations in the same order, so the same (face, bary) give the same bits.  `colors`,
  `texture` + `uv` and `bg` are `raster_shade`'s.  Where face is -1 (or names no face): normals 0, rgb = bg."""
  name = 'raycast_shade'
  verts, normals, faces = m['vertices'], m['normals'], m['faces']
  V, T = _mesh_tensors(name, verts, faces, normals, max_faces=2 ** 31 - 2)
  _chk(face, torch.int32, f'{name}: face')
  _chk(bary, f32, f'{name}: bary')
  if tuple(bary.shape) != tuple(face.shape) + (3,):
    raise ValueError(f'{name}: bary must be face\'s shape + [3], are {tuple(bary.shape)} and {tuple(face.shape)}')
  a = L.RasterArgs()
  a.verts, a.normals, a.faces, a.n_verts, a.n_faces = verts.data_ptr(), normals.data_ptr(), faces.data_ptr(), V, T
  _shade_colour_args(name, a, colors, texture, uv, bg)
  n = face.numel()
  out = dict(normals=torch.empty_like(bary), rgb=torch.empty_like(bary))
  L.check(lib().mnr_raycast_shade(C.byref(a), _ptr(face), _ptr(bary), n, _ptr(out['normals']), _ptr(out['rgb']), _stream()))
  return out


# ----------------------------------------------------------------------------- mesh registration (csrc/meshreg.hip)

def _chk_points(name, label, t, n=None):
  _chk(t, f32, f'{name}: {label}')
  if t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
    raise ValueError(f'{name}: {label} must be [{"N" if n is None else n},3], is {tuple(t.shape)}')
  if t.shape[0] >= 2 ** 31:
    raise ValueError(f'{name}: {t.shape[0]} points: must stay below 2^31')
  return int(t.shape[0])


def mesh_closest(points, face, verts, faces, vnormals=None):
  """(x [N,3], nrm [N,3]) float32: the closest point of face[i] (int32 [N], what `point_mesh_distance` returned; -1: none) to
  points[i] and that face's unit normal (mnr_mesh_closest; include/mnerf.h states every operation: x is the foot of the term of
  the distance formula that gave d2).  With `vnormals` [V,3] a face (i, i, i), a cloud's point, takes vnormals[i] normalised.
  Where face is -1 or names no valid face, or the point is not finite: x = the point itself, nrm = 0."""
  name = 'mesh_closest'
  N = _chk_points(name, 'points', points)
  V, T = _chk_mesh(name, verts, faces)
  _chk(face, torch.int32, f'{name}: face')
  if tuple(face.shape) != (N,):
    raise ValueError(f'{name}: face must be [{N}], is {tuple(face.shape)}')
  if vnormals is not None:
    _chk_points(name, 'vnormals', vnormals, V)
  x, nrm = torch.empty_like(points), torch.empty_like(points)
  L.check(lib().mnr_mesh_closest(_ptr(verts), V, _ptr(faces), T, _ptr(vnormals), _ptr(points), _ptr(face), N, _ptr(x), _ptr(nrm), _stream()))
  return x, nrm


def mesh_face_normals(verts, faces):
  """nrm [T,3] float32: the unit normals cross(b - a, c - a) / |.| of the faces (mnr_mesh_face_normals; include/mnerf.h), 0 for a
  face that is not valid or has no area."""
  V, T = _chk_mesh('mesh_face_normals', verts, faces)
  nrm = torch.empty((T, 3), dtype=f32, device=verts.device)
  L.check(lib().mnr_mesh_face_normals(_ptr(verts), V, _ptr(faces), T, _ptr(nrm), _stream()))
  return nrm


def icp_sums(p, x, nrm, keep, centre, out=None):
  """[ICP_SUMS = 47] float64 on the device: the sums of one ICP iteration over the correspondences with keep[i] != 0 (uint8 [N]), in
  float64 from p, x, nrm [N,3] float32 with `centre` (3 finite numbers) taken off p and x (mnr_icp_sums; include/mnerf.h fixes the
  layout: count, sum p', sum x', sum p' x'^T, sum |p'|^2, sum |x'|^2, sum |p - x|^2, sum r^2, the upper triangle of sum J^T J and
  sum J^T r).  Two fixed levels of reduction: two runs agree bit for bit."""
  name = 'icp_sums'
  N = _chk_points(name, 'p', p)
  _chk_points(name, 'x', x, N)
  _chk_points(name, 'nrm', nrm, N)
  _chk(keep, torch.uint8, f'{name}: keep')
  if tuple(keep.shape) != (N,):
    raise ValueError(f'{name}: keep must be [{N}], is {tuple(keep.shape)}')
  _chk(out, f64, f'{name}: out', allow_none=True)
  if out is None:
    out = torch.empty((L.ICP_SUMS,), dtype=f64, device=p.device)
  elif tuple(out.shape) != (L.ICP_SUMS,):
    raise ValueError(f'{name}: out must be [{L.ICP_SUMS}], is {tuple(out.shape)}')
  c = (C.c_double * 3)(*finite3(name, 'centre', centre))
  partials = torch.empty((max(lib().mnr_icp_sums_partials(N), 1),), dtype=f64, device=p.device)
  L.check(lib().mnr_icp_sums(N, _ptr(p), _ptr(x), _ptr(nrm), _ptr(keep), c, _ptr(partials), _ptr(out), _stream()))
  return out


def crop_polygon(points, polygon, axis, w_min, w_max):
  """keep [N] uint8: 1 where points[i] (float32 [N,3]) lies inside the prism of `polygon` [m,2] float64 (the corners' coordinates in
  the plane orthogonal to `axis`, 0 / 1 / 2 for X / Y / Z: (y, z), (x, z), (x, y)) between w_min and w_max along the axis, both ends
  included (mnr_crop_polygon; include/mnerf.h: even-odd crossing count in float64).  3 <= m <= CROP_MAX_POLYGON = 4096."""
  name = 'crop_polygon'
  N = _chk_points(name, 'points', points)
  _chk(polygon, f64, f'{name}: polygon')
  if polygon.dim() != 2 or polygon.shape[1] != 2 or not 3 <= polygon.shape[0] <= L.CROP_MAX_POLYGON:
    raise ValueError(f'{name}: polygon must be [m,2] with 3 <= m <= {L.CROP_MAX_POLYGON}, is {tuple(polygon.shape)}')
  if axis not in (0, 1, 2):
    raise ValueError(f'{name}: axis = {axis} must be 0, 1 or 2')
  w_min, w_max = float(w_min), float(w_max)
  if not (math.isfinite(w_min) and math.isfinite(w_max) and w_min <= w_max):
    raise ValueError(f'{name}: needs finite w_min <= w_max, are {w_min} and {w_max}')
  keep = torch.empty((N,), dtype=torch.uint8, device=points.device)
  L.check(lib().mnr_crop_polygon(_ptr(points), N, _ptr(polygon), int(polygon.shape[0]), int(axis), w_min, w_max, _ptr(keep), _stream()))
  return keep
