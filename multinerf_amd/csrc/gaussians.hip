// Integrated positional encoding of CALLER-SUPPLIED Gaussians -> bf16 feature rows (gfx950): the featurisation of a stand-alone
// MLP call (MLP.__call__(rng, gaussians=(means, covs), ...), reference models.py:403-409,441-446), where no ray exists.
//
// Per sample, in fp32:
//   coord.track_linearize(coord.contract)   (coord.py:21-27, 39-60) for a GENERAL symmetric covariance
//   coord.lift_and_diagonalize              (coord.py:129-133)
//   coord.integrated_pos_enc                (coord.py:102-126) with math.safe_sin (math.py:26-38)
// cast_rays_ipe_kernel (features.hip) evaluates the contraction from the structure of a ray's own Gaussian,
// cov = t_var d d^T + r_var (I - d d^T/|d|^2) (fe_gaussian, ipe_math.h), and the tangents of the density-gradient normals from the
// same structure (fe_contract_tangent); neither form exists for an arbitrary 3x3 covariance, so both are restated here.  Behind
// the Gaussian the two kernels evaluate the SAME separately rounded operations: the encoding loop, the LDS staging and the
// 16-byte-per-lane write-out below are a copy of cast_rays_ipe_kernel's (features.hip; that file's device code is pinned by
// profiles/r6_validated_isa.json, so the code is repeated rather than moved into a header), and on Gaussians exported by
// mnr_cast_rays_ipe without a contraction the rows are bit-identical to that kernel's.
//
// EXTENT OF THE COPY (a change to features.hip must be mirrored here): everything in ipe_from_gaussians_kernel behind phase 1,
// i.e. the encode loop (~40 lines), the padding loop and the write-out, the LDS layout in front of them, and gs_launch's
// argument checks, samples-per-block / pitch / LDS arithmetic (fe_launch): about 170 lines in all; GsTangent restates FeTangent.
// Nothing but tests/test_gpu_mlp_call.py::test_rows_equal_the_ray_kernels_bit_for_bit ties the two copies together.
//
// Work split inside a 256-thread block handling SPB consecutive samples (as in features.hip):
//   phase 1: one thread per sample: symmetrise, warp -> LDS
//   phase 2: one thread per (sample, basis direction): projection, then the L degrees
//   phase 3: all threads: coalesced copy of the [SPB, ld] rows to HBM
#include "common.h"

#pragma clang fp contract(off)

#define GS_THREADS 256
#define GS_STAGE_BYTES (32 * 1024)                      // feature rows a block stages in LDS
#include "ipe_math.h"

// d z / d mean_c and d (J cov J^T) / d mean_c of the contraction, covariance held fixed (c = x, y, z).
struct GsTangent {
  float dz[3][3];
  float dC[3][6];          // xx, xy, xz, yy, yz, zz
};

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
__device__ __forceinline__ void gs_contract(FeSample& g, GsTangent& T) {
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
__global__ __launch_bounds__(GS_THREADS) void ipe_from_gaussians_kernel(
    mnr_ipe_cfg c, int64_t total, int spb, int pitch, const float* __restrict__ means, const float* __restrict__ covs,
    const float* __restrict__ basis, void* __restrict__ feat_out, int ld_feat, float* __restrict__ means_out,
    float* __restrict__ covs_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int K = c.basis_k;
  const int L = c.max_deg - c.min_deg;
  const int nfeat = 2 * K * L;
  // LDS: samples [spb] FeSample | (TANGENT: [spb] GsTangent) | basis [K*3] | rows [spb][pitch] (x 3 if TANGENT)
  FeSample* gs = (FeSample*)smem;
  GsTangent* gt = (GsTangent*)(gs + spb);
  float* bs = TANGENT ? (float*)(gt + spb) : (float*)(gs + spb);
  char* rows = (char*)(bs + ((K * 3 + 3) & ~3));
  const int64_t s0 = (int64_t)blockIdx.x * spb;
  const int ns = (int)min((int64_t)spb, total - s0);

  for (int i = threadIdx.x; i < K * 3; i += GS_THREADS) bs[i] = basis[i];
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
    GsTangent T;
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

  // ---- from here on: cast_rays_ipe_kernel's encode loop, padding and write-out (features.hip), operation for operation ----
  const int row_elems = OUT_F32 ? nfeat : ld_feat;
  const float inv_k = 1.0f / (float)K;
  for (int pair = threadIdx.x; pair < ns * K; pair += GS_THREADS) {
    const int si = (int)(((float)pair + 0.5f) * inv_k);       // pair / K, exact for pair < 2^20
    const int k = pair - si * K;
    const FeSample g = gs[si];
    const float px = bs[k * 3 + 0], py = bs[k * 3 + 1], pz = bs[k * 3 + 2];
    // coord.py:131-132: mean . p_k ; p_k^T cov p_k.
    const float lm = g.mean[0] * px + g.mean[1] * py + g.mean[2] * pz;
    const float cx = g.cov[0] * px + g.cov[1] * py + g.cov[2] * pz;
    const float cy = g.cov[1] * px + g.cov[3] * py + g.cov[4] * pz;
    const float cz = g.cov[2] * px + g.cov[4] * py + g.cov[5] * pz;
    const float lv = px * cx + py * cy + pz * cz;
    const float vscale = -0.5f * 1.44269504088896340736f * lv;       // exp(-v/2) = exp2(vscale * 4^deg)
    char* rowp = rows + (size_t)si * pitch + (size_t)k * (OUT_F32 ? 4 : (int)sizeof(bf16));       // column k of the sample's row (row 0 of 3 if TANGENT)
    const int half = K * L * (OUT_F32 ? 4 : (int)sizeof(bf16));                      // byte offset of the cos half of the row
    const int lstep = K * (OUT_F32 ? 4 : (int)sizeof(bf16));
    float sc = ldexpf(1.0f, c.min_deg);                              // 2^deg, exact
    float sn = 0.0f, cs = 1.0f, att = 1.0f;
    float dlm[3] = {px, py, pz}, dlv[3] = {0.0f, 0.0f, 0.0f};
    if (TANGENT) {
      const GsTangent& T = gt[si];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        dlm[cc] = px * T.dz[cc][0] + py * T.dz[cc][1] + pz * T.dz[cc][2];
        const float* C6 = T.dC[cc];
        dlv[cc] = px * (C6[0] * px + C6[1] * py + C6[2] * pz) + py * (C6[1] * px + C6[3] * py + C6[4] * pz) +
                  pz * (C6[2] * px + C6[4] * py + C6[5] * pz);
      }
    }
    for (int l = 0; l < L; ++l) {
      if ((l & 3) == 0) {
        fe_sincos_wrapped(fe_wrap_100pi(lm * sc), &sn, &cs);
        att = exp2f(vscale * sc * sc);
      }
      const float fs = att * sn;
      const float fc = att * cs;
      if (TANGENT) {
        // d/d mean_c of att sin(lm 2^l) = att 2^l cos(.) dlm_c - 1/2 4^l att sin(.) dlv_c;  of att cos(.): -att 2^l sin(.) dlm_c
        // - 1/2 4^l att cos(.) dlv_c, with dlm_c = p_k . dz[c], dlv_c = p_k^T dC[c] p_k.
        const float hv = -0.5f * sc * sc;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          char* rp = rowp + (size_t)cc * spb * pitch;
          *(bf16*)rp = (bf16)(fc * sc * dlm[cc] + hv * fs * dlv[cc]);
          *(bf16*)(rp + half) = (bf16)(-fs * sc * dlm[cc] + hv * fc * dlv[cc]);
        }
      } else if (OUT_F32) {
        *(float*)rowp = fs;
        *(float*)(rowp + half) = fc;
      } else {
        const f32x2 pr = {fs, fc};
        const bf16x2 pb = __builtin_convertvector(pr, bf16x2);       // one v_cvt_pk_bf16_f32
        *(bf16*)rowp = pb[0];
        *(bf16*)(rowp + half) = pb[1];
      }
      rowp += lstep;
      const float s2 = 2.0f * sn * cs;
      cs = 1.0f - 2.0f * sn * sn;
      sn = s2;
      const float a2 = att * att;
      att = a2 * a2;
      sc *= 2.0f;
    }
  }
  if (!OUT_F32) {
    // zero the padding columns [nfeat, ld)
    const int pad = ld_feat - nfeat;
    const int nrows = TANGENT ? 3 * spb : ns;
    for (int e = threadIdx.x; e < nrows * pad; e += GS_THREADS) {
      const int si = e / pad, cidx = nfeat + e % pad;
      ((bf16*)(rows + (size_t)si * pitch))[cidx] = (bf16)0.0f;
    }
  }
  __syncthreads();
  // Coalesced write-out: the block's rows are contiguous in HBM (16 B per lane); in LDS they are `pitch` apart.
  const int row_bytes = row_elems * (OUT_F32 ? 4 : (int)sizeof(bf16));
  const int cpr = row_bytes >> 4;                         // 16-B chunks per row (row_bytes is a multiple of 16)
  for (int cc = 0; cc < (TANGENT ? 3 : 1); ++cc) {
    char* dst = (char*)feat_out + ((size_t)cc * total + s0) * row_bytes;
    const char* src = rows + (size_t)cc * spb * pitch;
    for (int ch = threadIdx.x; ch < ns * cpr; ch += GS_THREADS) {
      const int r = ch / cpr, o = (ch - r * cpr) << 4;
      *(uint4*)(dst + (size_t)r * row_bytes + o) = *(const uint4*)(src + (size_t)r * pitch + o);
    }
  }
}

// One launch: the argument checks and the block geometry of fe_launch (features.hip).
static int gs_launch(int mode /*0 bf16, 1 f32, 2 tangent*/, const char* who, const mnr_ipe_cfg* cfg, int64_t M, const float* means,
                     const float* covs, const float* basis, void* feat_out, int ld_feat, float* means_out, float* covs_out,
                     void* stream) {
  const int K = cfg->basis_k, L = cfg->max_deg - cfg->min_deg;
  MNR_CHECK_ARG(K >= 1 && K <= 128 && L >= 1 && L <= 32, "%s: basis_k=%d / degrees=%d out of range", who, K, L);
  const bool f32 = mode == 1;
  const bool tangent = mode == 2;
  const int nfeat = 2 * K * L;
  const int row_elems = f32 ? nfeat : ld_feat;
  MNR_CHECK_ARG(f32 || (ld_feat >= nfeat && ld_feat % 8 == 0), "%s: ld_feat=%d must be >= %d and a multiple of 8", who, ld_feat, nfeat);
  MNR_CHECK_ARG(!f32 || nfeat % 4 == 0, "%s: feature count must be a multiple of 4 for the fp32 rows", who);
  const size_t row_bytes = (size_t)row_elems * (f32 ? 4 : sizeof(bf16));
  int spb = (int)(GS_STAGE_BYTES / (row_bytes * (tangent ? 3 : 1)));
  if (spb > GS_THREADS) spb = GS_THREADS;
  spb &= ~3;                       // keeps the row buffer 16-byte aligned behind the FeSample array
  MNR_CHECK_ARG(spb >= 4, "%s: feature row too long", who);
  // 48 B of padding per staged row: consecutive samples then sit 12 banks apart
  const int pitch = (int)row_bytes + 48;
  const size_t lds = (size_t)spb * (sizeof(FeSample) + (tangent ? sizeof(GsTangent) : 0)) + (size_t)((K * 3 + 3) & ~3) * 4 +
                     (size_t)spb * pitch * (tangent ? 3 : 1);
  // (short rows: spb is capped by the thread count, not by the staging budget, and three tangent rows per sample plus their
  // padding can pass what a launch gets without raising the dynamic-LDS limit)
  MNR_CHECK_ARG(lds <= 64 * 1024, "%s: ld_feat=%d needs %zu bytes of LDS per block (limit 65536): use a longer row", who, ld_feat, lds);
  const int grid = mnr_cdiv(M, spb);
  if (tangent) {
    hipLaunchKernelGGL((ipe_from_gaussians_kernel<false, true>), dim3(grid), dim3(GS_THREADS), lds, (hipStream_t)stream, *cfg,
                       M, spb, pitch, means, covs, basis, feat_out, ld_feat, means_out, covs_out);
  } else if (f32) {
    hipLaunchKernelGGL((ipe_from_gaussians_kernel<true, false>), dim3(grid), dim3(GS_THREADS), lds, (hipStream_t)stream, *cfg,
                       M, spb, pitch, means, covs, basis, feat_out, ld_feat, means_out, covs_out);
  } else {
    hipLaunchKernelGGL((ipe_from_gaussians_kernel<false, false>), dim3(grid), dim3(GS_THREADS), lds, (hipStream_t)stream, *cfg,
                       M, spb, pitch, means, covs, basis, feat_out, ld_feat, means_out, covs_out);
  }
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_ipe_from_gaussians(const mnr_ipe_cfg* cfg, int64_t M, const float* means, const float* covs,
                                      const float* basis, void* feat_out, int ld_feat, float* feat_f32_out, float* means_out,
                                      float* covs_out, void* stream) {
  MNR_CHECK_ARG(cfg && M > 0 && means && covs && basis && feat_out, "mnr_ipe_from_gaussians: null argument");
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
