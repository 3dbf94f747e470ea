// Integrated positional encoding of CALLER-SUPPLIED Gaussians -> bf16 feature rows (gfx950): the featurisation of a stand-alone
// MLP call (MLP.__call__(rng, gaussians=(means, covs), ...), reference models.py:403-409,441-446), where no ray exists.
//
// Per sample, in fp32:
//   coord.track_linearize(coord.contract)   (coord.py:21-27, 39-60) for a GENERAL symmetric covariance
//   coord.lift_and_diagonalize              (coord.py:129-133)
//   coord.integrated_pos_enc                (coord.py:102-126) with math.safe_sin (math.py:26-38)
// cast_rays_ipe_kernel (features.hip) evaluates the contraction from the structure of a ray's own Gaussian,
// cov = t_var d d^T + r_var (I - d d^T/|d|^2) (fe_gaussian, ipe_math.h), and the tangents of the density-gradient normals from the
// same structure (fe_contract_tangent); neither form exists for an arbitrary 3x3 covariance.
//
// RESTATED here, for a general covariance: the contraction and its tangents (gs_contract), and phase 1 around them.
// SHARED with cast_rays_ipe_kernel: FeSample / FeTangent, the block size and the block geometry with its argument checks
// (fe_block_geometry, ipe_math.h), and everything behind phase 1 -- the encode loop, the LDS staging and the 16-byte-per-lane
// write-out (ipe_encode_body.inc, included textually by both kernels).  So behind the Gaussian the two kernels evaluate the SAME
// separately rounded operations, and on Gaussians exported by mnr_cast_rays_ipe without a contraction the rows are bit-identical
// to that kernel's (tests/test_gpu_mlp_call.py::test_rows_equal_the_ray_kernels_bit_for_bit).
//
// Work split inside a 256-thread block handling SPB consecutive samples (as in features.hip):
//   phase 1: one thread per sample: symmetrise, warp -> LDS
//   phase 2: one thread per (sample, basis direction): projection, then the L degrees     } ipe_encode_body.inc
//   phase 3: all threads: coalesced copy of the [SPB, ld] rows to HBM                     }
#include "common.h"

#pragma clang fp contract(off)

#include "ipe_math.h"

// coord.track_linearize(coord.contract) on (x, cov), cov = the six values xx, xy, xz, yy, yz, zz of a symmetric matrix:
// m = max(eps, |x|^2); identity for m <= 1; otherwise z = s x, J = s I + cc x x^T (symmetric), s = (2 sqrt(m) - 1)/m,
// cc = 2 (1 - sqrt(m))/m^2, and with w = cov x
//   J cov J = s^2 cov + s cc (x w^T + w x^T) + cc^2 (x.w) x x^T.
// TANGENT: with the covariance an input held fixed (what jax.value_and_grad(predict_density) differentiates, models.py:441-446,
// 473-492), dz_c = column c of J and dC_c = dJ_c cov J + J cov dJ_c = A_c + A_c^T, A_c = dJ_c (cov J),
//   dJ_c = ds_c I + dcc_c x x^T + cc (e_c x^T + x e_c^T),  ds_c = cc x_c,  dcc_c = 2 cc' x_c,  cc' = (3 sqrt(m) - 4)/m^3,
//   cov J = s cov + cc w x^T,   x^T cov J = s w^T + cc (x.w) x^T.
// Inside the unit ball dz_c = e_c and dC_c = 0.
template <bool TANGENT>
__device__ __forceinline__ void gs_contract(FeSample& g, FeTangent& T) {
  const int ii[6] = {0, 0, 0, 1, 1, 2}, jj[6] = {0, 1, 2, 1, 2, 2};
  if (TANGENT) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int i = 0; i < 3; ++i) T.dz[c][i] = (i == c) ? 1.0f : 0.0f;
#pragma unroll
      for (int e = 0; e < 6; ++e) T.dC[c][e] = 0.0f;
    }
  }
  const float x[3] = {g.mean[0], g.mean[1], g.mean[2]};
  const float m = fmaxf(MNR_F32_EPS, x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (m <= 1.0f) return;
  const float sq = sqrtf(m);
  const float s = (2.0f * sq - 1.0f) / m;
  const float cc = 2.0f * (1.0f - sq) / (m * m);
  const float cv[3][3] = {{g.cov[0], g.cov[1], g.cov[2]}, {g.cov[1], g.cov[3], g.cov[4]}, {g.cov[2], g.cov[4], g.cov[5]}};
  float w[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = cv[i][0] * x[0] + cv[i][1] * x[1] + cv[i][2] * x[2];
  const float xw = x[0] * w[0] + x[1] * w[1] + x[2] * w[2];
  if (TANGENT) {
    const float ccp = (3.0f * sq - 4.0f) / (m * m * m);            // d cc / d m
    float Bm[3][3], xB[3];                                          // cov J and x^T cov J
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      xB[i] = s * w[i] + cc * xw * x[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) Bm[i][j] = s * cv[i][j] + cc * w[i] * x[j];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float ds = cc * x[c];
      const float dcc = 2.0f * ccp * x[c];
      float A[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        T.dz[c][i] = cc * x[c] * x[i] + (i == c ? s : 0.0f);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          A[i][j] = ds * Bm[i][j] + dcc * x[i] * xB[j] + cc * ((i == c ? xB[j] : 0.0f) + x[i] * Bm[c][j]);
      }
#pragma unroll
      for (int e = 0; e < 6; ++e) T.dC[c][e] = A[ii[e]][jj[e]] + A[jj[e]][ii[e]];
    }
  }
  const float s2 = s * s, scc = s * cc, c2xw = cc * cc * xw;
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const int i = ii[e], j = jj[e];
    g.cov[e] = s2 * cv[i][j] + scc * (x[i] * w[j] + w[i] * x[j]) + c2xw * x[i] * x[j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) g.mean[i] = s * x[i];
}

template <bool OUT_F32, bool TANGENT>
__global__ __launch_bounds__(FE_THREADS) void ipe_from_gaussians_kernel(
    mnr_ipe_cfg c, int64_t total, int spb, int pitch, const float* __restrict__ means, const float* __restrict__ covs,
    const float* __restrict__ basis, void* __restrict__ feat_out, int ld_feat, float* __restrict__ means_out,
    float* __restrict__ covs_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int K = c.basis_k;
  const int L = c.max_deg - c.min_deg;
  const int nfeat = 2 * K * L;
  // LDS: samples [spb] FeSample | (TANGENT: [spb] FeTangent) | basis [K*3] | rows [spb][pitch] (x 3 if TANGENT)
  FeSample* gs = (FeSample*)smem;
  FeTangent* gt = (FeTangent*)(gs + spb);
  float* bs = TANGENT ? (float*)(gt + spb) : (float*)(gs + spb);
  char* rows = (char*)(bs + ((K * 3 + 3) & ~3));
  const int64_t s0 = (int64_t)blockIdx.x * spb;
  const int ns = (int)min((int64_t)spb, total - s0);

  for (int i = threadIdx.x; i < K * 3; i += FE_THREADS) bs[i] = basis[i];
  if (threadIdx.x < ns) {
    const int64_t s = s0 + threadIdx.x;
    float cf[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) cf[i] = covs[s * 9 + i];
    FeSample g;
#pragma unroll
    for (int i = 0; i < 3; ++i) g.mean[i] = means[s * 3 + i];
    // Symmetrise exactly the way diag(P^T C P) sees it (fe_gaussian): keep both triangles' average.
    g.cov[0] = cf[0];
    g.cov[1] = 0.5f * (cf[1] + cf[3]);
    g.cov[2] = 0.5f * (cf[2] + cf[6]);
    g.cov[3] = cf[4];
    g.cov[4] = 0.5f * (cf[5] + cf[7]);
    g.cov[5] = cf[8];
    FeTangent T;
    if (c.warp_contract) {
      gs_contract<TANGENT>(g, T);
    } else if (TANGENT) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
#pragma unroll
        for (int i = 0; i < 3; ++i) T.dz[cc][i] = (i == cc) ? 1.0f : 0.0f;
#pragma unroll
        for (int e = 0; e < 6; ++e) T.dC[cc][e] = 0.0f;
      }
    }
    gs[threadIdx.x] = g;
    if (TANGENT) gt[threadIdx.x] = T;
    if (means_out) {
#pragma unroll
      for (int i = 0; i < 3; ++i) means_out[s * 3 + i] = g.mean[i];
    }
    if (covs_out) {
      const float* cv = g.cov;
      const float full[9] = {cv[0], cv[1], cv[2], cv[1], cv[3], cv[4], cv[2], cv[4], cv[5]};
#pragma unroll
      for (int i = 0; i < 9; ++i) covs_out[s * 9 + i] = full[i];
    }
  }
  __syncthreads();

#include "ipe_encode_body.inc"
}

static int gs_launch(int mode /*0 bf16, 1 f32, 2 tangent*/, const char* who, const mnr_ipe_cfg* cfg, int64_t M, const float* means,
                     const float* covs, const float* basis, void* feat_out, int ld_feat, float* means_out, float* covs_out,
                     void* stream) {
  FeGeometry geo;                  // (fp32 rows: mnr_ipe_from_gaussians' second pass only)
  const int st = fe_block_geometry(who, "mnr_ipe_from_gaussians: feature count must be a multiple of 4 for the fp32 rows", cfg, mode,
                                   ld_feat, &geo);
  if (st != MNR_OK) return st;         // (includes the refusal of a block that needs more than 64 KiB of LDS, as for fe_launch, features.hip)
  const dim3 grid(mnr_cdiv(M, geo.spb)), block(FE_THREADS);
  if (mode == 2) {
    hipLaunchKernelGGL((ipe_from_gaussians_kernel<false, true>), grid, block, geo.lds, (hipStream_t)stream, *cfg, M, geo.spb,
                       geo.pitch, means, covs, basis, feat_out, ld_feat, means_out, covs_out);
  } else if (mode == 1) {
    hipLaunchKernelGGL((ipe_from_gaussians_kernel<true, false>), grid, block, geo.lds, (hipStream_t)stream, *cfg, M, geo.spb,
                       geo.pitch, means, covs, basis, feat_out, ld_feat, means_out, covs_out);
  } else {
    hipLaunchKernelGGL((ipe_from_gaussians_kernel<false, false>), grid, block, geo.lds, (hipStream_t)stream, *cfg, M, geo.spb,
                       geo.pitch, means, covs, basis, feat_out, ld_feat, means_out, covs_out);
  }
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_ipe_from_gaussians(const mnr_ipe_cfg* cfg, int64_t M, const float* means, const float* covs,
                                      const float* basis, void* feat_out, int ld_feat, float* feat_f32_out, float* means_out,
                                      float* covs_out, void* stream) {
  MNR_CHECK_ARG(cfg && M > 0 && means && covs && basis && feat_out, "mnr_ipe_from_gaussians: null argument");
  // (the second pass's own refusal, ahead of the first launch: a refused call writes nothing)
  MNR_CHECK_ARG(!feat_f32_out || (2 * cfg->basis_k * (cfg->max_deg - cfg->min_deg)) % 4 == 0,
                "mnr_ipe_from_gaussians: feature count must be a multiple of 4 for the fp32 rows");
  int st = gs_launch(0, "mnr_ipe_from_gaussians", cfg, M, means, covs, basis, feat_out, ld_feat, means_out, covs_out, stream);
  if (st != MNR_OK || !feat_f32_out) return st;
  // the parity-test leaf: the same features unrounded, [M, 2KL] without padding, from a second pass over the Gaussians
  return gs_launch(1, "mnr_ipe_from_gaussians", cfg, M, means, covs, basis, feat_f32_out, 0, nullptr, nullptr, stream);
}

extern "C" int mnr_ipe_from_gaussians_tangent(const mnr_ipe_cfg* cfg, int64_t M, const float* means, const float* covs,
                                              const float* basis, void* feat_out, int ld_feat, void* stream) {
  MNR_CHECK_ARG(cfg && M > 0 && means && covs && basis && feat_out, "mnr_ipe_from_gaussians_tangent: null argument");
  return gs_launch(2, "mnr_ipe_from_gaussians_tangent", cfg, M, means, covs, basis, feat_out, ld_feat, nullptr, nullptr, stream);
}
