// Per-sample Gaussian and trigonometric helpers of the integrated positional encoding, shared by the stand-alone
// featurisation kernel of rays (features.hip), that of caller-supplied Gaussians (gaussians.hip) and the fused chain's in-kernel
// layer-0 producer (fused_mlp.hip); the two featurisation kernels also share their block geometry (fe_block_geometry below)
// and everything behind the per-sample Gaussian (ipe_encode_body.inc).
//
// Include it with floating-point contraction switched OFF (#pragma clang fp contract(off) in front of the include): all
// users must evaluate the same separately rounded operations, or the features the fused chain builds in LDS and the rows of
// ipe_from_gaussians_kernel stop being bit-identical to the rows cast_rays_ipe_kernel writes (the explicit fmaf calls are
// fused in all).
#pragma once

#include "common.h"

// Block size and LDS staging budget of cast_rays_ipe_kernel and ipe_from_gaussians_kernel.
#ifndef FE_THREADS                                     // (probe builds: -DFE_THREADS=... -DFE_STAGE_BYTES=..., tools/ipe_probe.py)
#define FE_THREADS 256
#endif
#ifndef FE_STAGE_BYTES
#define FE_STAGE_BYTES (32 * 1024)                      // feature rows a block stages in LDS
#endif

#define FE_PI_2 1.57079632679489661923f
#define FE_100PI 314.159265358979323846f

__device__ __forceinline__ float fe_safe_sin(float x) {
  // math.py:26-28: sin(x if |x| < 100*pi else x mod 100*pi); `%` takes the divisor's sign.
  const float t = FE_100PI;
  if (!(fabsf(x) < t)) {
    float m = fmodf(x, t);
    if (m != 0.0f && (m < 0.0f)) m += t;
    x = m;
  }
  return sinf(x);
}

// math.safe_sin's argument wrap (math.py:26-28): y if |y| < 100 pi, else y mod 100 pi with the divisor's sign -- the value
// cast_rays_ipe_kernel gets from fmodf, without the library call's ~150-instruction loop (the fused chain's in-kernel
// encoding is bound by its instruction stream, not by HBM).  fmod is exact, so it can be had from one FMA: with q the
// truncated quotient, y - q t is representable and fmaf(-q, t, y) returns it unrounded.  q comes from a multiplication by
// 1/t (|error| < 0.2 for |y| < 1e8, i.e. off by at most one, and only next to a multiple of t): a quotient one too large
// shows as a remainder of the wrong sign, one too small as |r| >= t (rounding is monotonic and t is representable), and
// the remainder is then taken again from y with the corrected quotient.  Bit-identical to the fmodf path.
__device__ __forceinline__ float fe_wrap_100pi(float y) {
  const float t = FE_100PI;
  if (!(fabsf(y) < t)) {
    float m;
    if (fabsf(y) < 1e8f) {
      const float qf = truncf(y * (1.0f / FE_100PI));
      m = fmaf(-qf, t, y);
      const float toward0 = qf - copysignf(1.0f, y), away = qf + copysignf(1.0f, y);
      if ((y > 0.0f) ? (m < 0.0f) : (m > 0.0f)) m = fmaf(-toward0, t, y);
      else if (fabsf(m) >= t) m = fmaf(-away, t, y);
    } else {
      m = fmodf(y, t);
    }
    if (m != 0.0f && (m < 0.0f)) m += t;
    y = m;
  }
  return y;
}

// sin and cos of y for |y| <= 100 pi (the argument after math.safe_sin's wrap): Cody-Waite reduction by pi/2 in three parts
// (k <= 200: k * FE_PIO2_A is exact), Cephes single-precision kernels on [-pi/4, pi/4] (|error| ~1e-7, the features then go to
// bf16).  ~20 VALU operations without a branch; the library sincosf carries its large-argument reduction along.
#define FE_PIO2_A 1.5703125f
#define FE_PIO2_B 4.837512969970703125e-4f
#define FE_PIO2_C 7.54978995489188216e-8f
__device__ __forceinline__ void fe_sincos_wrapped(float y, float* sn, float* cs) {
  const float kf = rintf(y * 0.63661977236758134308f);
  const int q = (int)kf;
  float r = fmaf(-kf, FE_PIO2_A, y);
  r = fmaf(-kf, FE_PIO2_B, r);
  r = fmaf(-kf, FE_PIO2_C, r);
  const float z = r * r;
  const float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
  const float s = fmaf(r * z, ps, r);
  const float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
  const float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
  const float a = (q & 1) ? c : s, b = (q & 1) ? s : c;
  *sn = (q & 2) ? -a : a;
  *cs = ((q + 1) & 2) ? -b : b;
}

struct FeSample {
  float mean[3];
  float cov[6];   // xx, xy, xz, yy, yz, zz (symmetric)
};

// d z / d mean_c and d (J cov J^T) / d mean_c of the contraction, covariance held fixed (c = x, y, z): the tangents behind the
// density-gradient normals.  Filled by fe_contract_tangent (features.hip: a ray's structured covariance) or gs_contract
// (gaussians.hip: a general one); identity / zero without a contraction and inside the unit ball.
struct FeTangent {
  float dz[3][3];
  float dC[3][6];          // xx, xy, xz, yy, yz, zz
};

// coord.py:131-132 for one basis direction p: lm = mean . p, lv = p^T cov p.
__device__ __forceinline__ void fe_project(const FeSample& g, float px, float py, float pz, float* lm, float* lv) {
  *lm = g.mean[0] * px + g.mean[1] * py + g.mean[2] * pz;
  const float cx = g.cov[0] * px + g.cov[1] * py + g.cov[2] * pz;
  const float cy = g.cov[1] * px + g.cov[3] * py + g.cov[4] * pz;
  const float cz = g.cov[2] * px + g.cov[4] * py + g.cov[5] * pz;
  *lv = px * cx + py * cy + pz * cz;
}

// The same for the tangent of mean component cc: dlm = p . dz[cc], dlv = p^T dC[cc] p.
__device__ __forceinline__ void fe_project_tangent(const FeTangent& T, int cc, float px, float py, float pz, float* dlm, float* dlv) {
  *dlm = px * T.dz[cc][0] + py * T.dz[cc][1] + pz * T.dz[cc][2];
  const float* C6 = T.dC[cc];
  *dlv = px * (C6[0] * px + C6[1] * py + C6[2] * pz) + py * (C6[1] * px + C6[3] * py + C6[4] * pz) +
         pz * (C6[2] * px + C6[4] * py + C6[5] * pz);
}

// Anchor of the degree loop (every 4th degree): sin / cos of the wrapped argument lm 2^l and the attenuation
// exp(-lv 4^l / 2) = exp2(vscale 4^l), sc = 2^l.
__device__ __forceinline__ void fe_anchor(float lm, float vscale, float sc, float* sn, float* cs, float* att) {
  fe_sincos_wrapped(fe_wrap_100pi(lm * sc), sn, cs);
  *att = exp2f(vscale * sc * sc);
}

// One degree up: the double-angle recurrence, att(l+1) = att(l)^4, sc = 2^(l+1).
__device__ __forceinline__ void fe_degree_step(float* sn, float* cs, float* att, float* sc) {
  const float s2 = 2.0f * *sn * *cs;
  *cs = 1.0f - 2.0f * *sn * *sn;
  *sn = s2;
  const float a2 = *att * *att;
  *att = a2 * a2;
  *sc *= 2.0f;
}

// Block geometry and the argument checks that go with it, for the launches of cast_rays_ipe_kernel (features.hip) and
// ipe_from_gaussians_kernel (gaussians.hip): mode 0 = bf16 rows [ld_feat], 1 = fp32 rows [2KL], 2 = three bf16 tangent rows per
// sample.  `who` names the entry in the messages; `f32_msg` is the whole refusal of fp32 rows that are no multiple of 16 bytes.
struct FeGeometry {
  int spb;        // samples per block
  int pitch;      // bytes between staged rows in LDS
  size_t lds;     // dynamic LDS bytes
};

static inline int fe_block_geometry(const char* who, const char* f32_msg, const mnr_ipe_cfg* cfg, int mode, int ld_feat,
                                    FeGeometry* geo) {
  const int K = cfg->basis_k, L = cfg->max_deg - cfg->min_deg;
  MNR_CHECK_ARG(K >= 1 && K <= 128 && L >= 1 && L <= 32, "%s: basis_k=%d / degrees=%d out of range", who, K, L);
  const bool f32 = mode == 1;
  const bool tangent = mode == 2;
  const int nfeat = 2 * K * L;
  const int row_elems = f32 ? nfeat : ld_feat;
  MNR_CHECK_ARG(f32 || (ld_feat >= nfeat && ld_feat % 8 == 0), "%s: ld_feat=%d must be >= %d and a multiple of 8", who, ld_feat, nfeat);
  MNR_CHECK_ARG(!f32 || nfeat % 4 == 0, "%s", f32_msg);
  const size_t row_bytes = (size_t)row_elems * (f32 ? 4 : sizeof(bf16));
  int spb = (int)(FE_STAGE_BYTES / (row_bytes * (tangent ? 3 : 1)));
  if (spb > FE_THREADS) spb = FE_THREADS;
  spb &= ~3;                       // keeps the row buffer 16-byte aligned behind the FeSample array
  MNR_CHECK_ARG(spb >= 4, "%s: feature row too long", who);
  // 48 B of padding per staged row: consecutive samples then sit 12 banks apart (a wave covers ~3 samples x 21 directions)
  geo->spb = spb;
  geo->pitch = (int)row_bytes + 48;
  geo->lds = (size_t)spb * (sizeof(FeSample) + (tangent ? sizeof(FeTangent) : 0)) + (size_t)((K * 3 + 3) & ~3) * 4 +
             (size_t)spb * geo->pitch * (tangent ? 3 : 1);
  // Short rows: spb is capped by the thread count, not by the staging budget, and three tangent rows per sample plus their
  // padding can pass what a launch gets without raising the dynamic-LDS limit (tangent rows of ld_feat <= 40).  Refused here,
  // for both launchers alike.
  MNR_CHECK_ARG(geo->lds <= 64 * 1024, "%s: ld_feat=%d needs %zu bytes of LDS per block (limit 65536): use a longer row", who, ld_feat,
                geo->lds);
  return MNR_OK;
}

__device__ __forceinline__ void fe_gaussian(const mnr_ipe_cfg& c, float t0, float t1, const float* o,
                                            const float* d, float radius, FeSample& g) {
  float t_mean, t_var, r_var;
  if (c.ray_shape == 0) {
    // render.py:62-70 (stable form of mip-NeRF eq. 7).
    const float mu = (t0 + t1) / 2.0f;
    const float hw = (t1 - t0) / 2.0f;
    const float denom = fmaxf(MNR_F32_EPS, 3.0f * mu * mu + hw * hw);
    const float hw2 = hw * hw, hw4 = hw2 * hw2;
    t_mean = mu + (2.0f * mu * hw2) / denom;
    t_var = hw2 / 3.0f - (4.0f / 15.0f) * hw4 * (12.0f * mu * mu - hw2) / (denom * denom);
    r_var = (mu * mu) / 4.0f + (5.0f / 12.0f) * hw2 - (4.0f / 15.0f) * hw4 / denom;
    r_var *= radius * radius;
  } else {
    // render.py:97-99.
    t_mean = (t0 + t1) / 2.0f;
    r_var = radius * radius / 4.0f;
    t_var = (t1 - t0) * (t1 - t0) / 12.0f;
  }
  // render.py:23-41 lift_gaussian(diag=False) and :126 (+ origins).
  const float dmag = fmaxf(1e-10f, d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  float mean[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) mean[i] = o[i] + d[i] * t_mean;
  float cov[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float dd = d[i] * d[j];
      const float null_outer = (i == j ? 1.0f : 0.0f) - d[i] * (d[j] / dmag);
      cov[i][j] = t_var * dd + r_var * null_outer;
    }
  if (c.disable_integration) {
    t_var = 0.0f;
    r_var = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) cov[i][j] = 0.0f;
  }
  if (c.warp_contract) {
    // coord.py:21-27 and its Jacobian (what jax.linearize yields, coord.py:58-59): identity inside
    // the unit ball; outside z = s x, J = s I + cc x x^T, s = (2 sqrt(m) - 1)/m, cc = 2 (1 - sqrt(m))/m^2.
    //
    // J cov J^T is evaluated from the STRUCTURE of cov = t_var d d^T + r_var (I - d d^T/|d|^2):
    //   J cov J^T = t_var u u^T + r_var (J^2 - u u^T/|d|^2),   u = J d,
    //   J^2 = s^2 I + (2 cc / sqrt(m)) x x^T            (2 s cc + cc^2 m = 2 cc / sqrt(m)),
    //   u   = [m - 2 (1 - sqrt(m)) (|o|^2 + t (o.d))] / m^2 * d + cc (x.d) o     (x = o + t d).
    // Same function as the reference's two matrix products, but without forming s*t_var*d d^T
    // (~1e5 for the far samples of 360.gin) only to cancel it against cc*(x.d)*t_var*x d^T: the
    // plain products lose ~10% of the tangential variance there in fp32.
    const float m = fmaxf(MNR_F32_EPS, mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2]);
    if (!(m <= 1.0f)) {
      const float sq = sqrtf(m);
      const float s = (2.0f * sq - 1.0f) / m;
      const float cc = 2.0f * (1.0f - sq) / (m * m);
      const float oo = o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
      const float od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2];
      const float xd = mean[0] * d[0] + mean[1] * d[1] + mean[2] * d[2];
      const float brk = (m - 2.0f * (1.0f - sq) * (oo + t_mean * od)) / (m * m);
      float u[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) u[i] = brk * d[i] + cc * xd * o[i];
      const float j2x = 2.0f * cc / sq;
      const float ku = t_var - r_var / dmag;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          cov[i][j] = ku * u[i] * u[j] + r_var * ((i == j ? s * s : 0.0f) + j2x * mean[i] * mean[j]);
#pragma unroll
      for (int i = 0; i < 3; ++i) mean[i] = s * mean[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) g.mean[i] = mean[i];
  // Symmetrise exactly the way diag(P^T C P) sees it: keep both triangles' average.
  g.cov[0] = cov[0][0];
  g.cov[1] = 0.5f * (cov[0][1] + cov[1][0]);
  g.cov[2] = 0.5f * (cov[0][2] + cov[2][0]);
  g.cov[3] = cov[1][1];
  g.cov[4] = 0.5f * (cov[1][2] + cov[2][1]);
  g.cov[5] = cov[2][2];
}
