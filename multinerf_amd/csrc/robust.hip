// RobustNeRF data loss on device (gfx950): the inlier mask and the threshold it is compared against.
//
// Replaces robustnerf.robustnerf_mask (robustnerf.py:8-86) with _robustnerf_inner_patch_mask (:89-115) as called from
// train_utils.compute_data_loss (train_utils.py:104-108), and the jnp.quantile (robustnerf.py:26-28) that train.py:128-129
// carries into the next step.  The reference builds [n,h,w,1] float images, a lax.conv and two broadcasts; a batch is
// num_patches * P * P pixels in [patch][y][x] order, so here one workgroup owns one patch: its inlier flags sit in LDS,
// the f x f vote reads them from there, the patch vote is a ballot per wave and a sum over the waves.  Votes are counted
// in integers and compared as count / n in double, the values the reference's float means take.  The quantile is an
// exact radix select over the float bit patterns in one workgroup.  Nothing comes back to the host: the threshold is a
// device scalar from one step to the next.
#include "common.h"

#define RB_MAX_THREADS 1024
#define RB_MAX_WAVES (RB_MAX_THREADS / 64)

// sum over the workgroup of one integer per wave (lane 0 of each wave holds it); every thread gets the total
__device__ __forceinline__ int rb_block_count(bool pred, int* slot, int wave, int lane, int nwaves) {
  const int c = __popcll(__ballot(pred ? 1 : 0));
  if (lane == 0) slot[wave] = c;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < nwaves; ++w) s += slot[w];
  return s;
}

__global__ __launch_bounds__(RB_MAX_THREADS) void robustnerf_mask_kernel(mnr_robust_args a, int num_patches) {
  __shared__ unsigned char l_in[RB_MAX_THREADS];           // (error < threshold) of this patch, [y][x]
  __shared__ int l_cnt[4][RB_MAX_WAVES];
  __shared__ double l_sq[RB_MAX_THREADS];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, nwaves = (int)blockDim.x >> 6;
  const int P = a.patch_size, n = P * P;
  if ((int)blockIdx.x >= num_patches) {
    // the padding rays behind B_valid: masked out
    const int64_t ray = a.B_valid + (int64_t)((int)blockIdx.x - num_patches) * blockDim.x + t;
    if (ray < a.B) {
      a.mask[ray] = 0.0f;
      if (a.lossmult_out) {
        for (int c = 0; c < a.lm_c; ++c) a.lossmult_out[ray * a.lm_c + c] = 0.0f;
      }
    }
    return;
  }
  const bool live = t < n;
  const int64_t ray = (int64_t)blockIdx.x * n + t;
  const int y = t / P, x = t - y * P;
  float w[3] = {0.0f, 0.0f, 0.0f};
  float err = 0.0f;
  double sq = 0.0;
  if (live) {
    float d2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = a.rgb[ray * 3 + c] - a.gt[ray * 3 + c];
      d2[c] = d * d;
      w[c] = a.lm_c == 1 ? a.lossmult[ray] : a.lossmult[ray * 3 + c];
      sq += (double)w[c] * (double)d2[c];                    // train_utils.py:86-88
    }
    err = (d2[0] + d2[1] + d2[2]) / 3.0f;                    // robustnerf.py:25
    if (a.err) a.err[ray] = err;
  }
  const bool inl = live && a.enable && err < *a.loss_threshold;      // robustnerf.py:39
  l_in[t] = inl ? 1 : 0;
  l_sq[t] = sq;
  const int n_inl = rb_block_count(inl, l_cnt[0], wave, lane, nwaves);   // (its barrier publishes l_in and l_sq too)
  bool has = false;
  if (live && a.enable) {
    // robustnerf.py:43-55: box filter with zero padding, then "more than 1 - q of the window"
    const int f = a.filter_size, h = f >> 1;
    int votes = 0;
    for (int dy = -h; dy <= h; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= P) continue;
      for (int dx = -h; dx <= h; ++dx) {
        const int xx = x + dx;
        if (xx >= 0 && xx < P) votes += l_in[yy * P + xx];
      }
    }
    has = (double)votes / (double)(f * f) > 1.0 - a.smoothed_inlier_quantile;
  }
  const int n_has = rb_block_count(has, l_cnt[1], wave, lane, nwaves);
  const bool pixel = has || inl;                                         // :57-59
  const int n_pixel = rb_block_count(pixel, l_cnt[2], wave, lane, nwaves);
  // :65-76: the whole inner square is switched on by the patch's vote
  const int lo = (P - a.inner_patch_size) / 2, hi = lo + a.inner_patch_size;
  const bool patch_in = a.enable && (double)n_pixel / (double)n > 1.0 - a.inner_patch_inlier_quantile;
  const bool inner = live && patch_in && y >= lo && y < hi && x >= lo && x < hi;
  const bool m = live && (a.enable ? (inner || pixel) : true);           // :81-83, :29
  const int n_mask = rb_block_count(m, l_cnt[3], wave, lane, nwaves);
  if (live) {
    const float mf = m ? 1.0f : 0.0f;
    a.mask[ray] = mf;
    if (a.lossmult_out) {
      if (a.lm_c == 1) {
        a.lossmult_out[ray] = w[0] * mf;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.lossmult_out[ray * 3 + c] = w[c] * mf;
      }
    }
  }
  if (a.mse && lane == 0) {
    double s = 0.0;
    for (int i = 0; i < 64; ++i) s += l_sq[wave * 64 + i];
    l_sq[wave * 64] = s;
  }
  __syncthreads();
  if (t == 0) {
    if (a.stats) {
      const double bv = (double)a.B_valid;
      if (a.enable) {
        const int n_inner = patch_in ? a.inner_patch_size * a.inner_patch_size : 0;
        unsafeAtomicAdd(a.stats + 0, (float)((double)n_inl / bv));
        unsafeAtomicAdd(a.stats + 1, (float)((double)n_has / bv));
        unsafeAtomicAdd(a.stats + 2, (float)((double)n_inner / bv));
      }
      unsafeAtomicAdd(a.stats + 3, (float)((double)n_mask / bv));
    }
    if (a.mse) {
      double s = 0.0;
      for (int wv = 0; wv < nwaves; ++wv) s += l_sq[wv * 64];
      unsafeAtomicAdd(a.mse, (float)(s / (double)*a.denom));
    }
  }
}

extern "C" int mnr_robustnerf_mask(const mnr_robust_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->B > 0 && a->B_valid > 0 && a->B_valid <= a->B, "mnr_robustnerf_mask: bad batch sizes");
  MNR_CHECK_ARG(a->rgb && a->gt && a->lossmult && a->loss_threshold && a->mask && (a->lm_c == 1 || a->lm_c == 3),
                "mnr_robustnerf_mask: needs rgb, gt, lossmult [B,1|3], loss_threshold and mask");
  MNR_CHECK_ARG(!a->mse || a->denom, "mnr_robustnerf_mask: the mse needs denom");
  const int P = a->patch_size;
  MNR_CHECK_ARG(P >= 1 && P * P <= RB_MAX_THREADS, "mnr_robustnerf_mask: patch_size^2 = %d exceeds the limit of %d pixels per patch",
                P * P, RB_MAX_THREADS);
  MNR_CHECK_ARG(a->filter_size >= 1 && (a->filter_size & 1) && a->filter_size <= P,
                "mnr_robustnerf_mask: robustnerf_smoothed_filter_size %d must be odd and at most patch_size %d", a->filter_size, P);
  MNR_CHECK_ARG(a->inner_patch_size >= 0 && a->inner_patch_size <= P,
                "mnr_robustnerf_mask: robustnerf_inner_patch_size %d must be at most patch_size %d", a->inner_patch_size, P);
  MNR_CHECK_ARG(a->B_valid % (P * P) == 0, "mnr_robustnerf_mask: B_valid %lld is not a multiple of patch_size^2 = %d",
                (long long)a->B_valid, P * P);
  MNR_CHECK_ARG(a->B_valid / (P * P) + a->B / 64 + 1 < (1ll << 30), "mnr_robustnerf_mask: batch too large");
  const int num_patches = (int)(a->B_valid / (P * P));
  const int threads = mnr_cdiv(P * P, 64) * 64;
  const int pad_blocks = mnr_cdiv(a->B - a->B_valid, threads);
  hipLaunchKernelGGL(robustnerf_mask_kernel, dim3(num_patches + pad_blocks), dim3(threads), 0, (hipStream_t)stream, *a,
                     num_patches);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// quantile: most-significant-digit radix select, 8 bits a pass, one workgroup.  Keys are the float bit patterns in their
// total order (sign flipped for positive values, all bits for negative ones), so any finite input selects exactly.

#define RQ_THREADS 1024
#define RQ_WAVES (RQ_THREADS / 64)

__device__ __forceinline__ unsigned rq_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rq_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool rq_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(RQ_THREADS) void quantile_kernel(int64_t N, const float* __restrict__ x, double q, float* out) {
  __shared__ unsigned l_hist[RQ_WAVES][256];               // one histogram per wave: LDS atomics collide inside a wave only
  __shared__ unsigned l_red[RQ_WAVES];
  __shared__ unsigned l_sel[4];                            // key prefix, rank inside it, size of the chosen bin, finite count
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  int c = 0;
  for (int64_t i = t; i < N; i += RQ_THREADS) c += rq_finite(x[i]) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if (lane == 0) l_red[wave] = (unsigned)c;
  __syncthreads();
  if (t == 0) {
    unsigned M = 0;
    for (int w = 0; w < RQ_WAVES; ++w) M += l_red[w];
    l_sel[3] = M;
    if (M == 0) {
      *out = __uint_as_float(0x7fc00000u);
    } else {
      double k = floor(q * (double)(M - 1));
      k = fmin(fmax(k, 0.0), (double)(M - 1));
      l_sel[0] = 0;
      l_sel[1] = (unsigned)k;
    }
  }
  __syncthreads();
  const unsigned M = l_sel[3];
  if (M == 0) return;
  unsigned digits = 0;                                     // mask of the key bits already chosen
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = t; b < RQ_WAVES * 256; b += RQ_THREADS) (&l_hist[0][0])[b] = 0;
    __syncthreads();
    const unsigned prefix = l_sel[0];
    for (int64_t i = t; i < N; i += RQ_THREADS) {
      const float v = x[i];
      const unsigned key = rq_key(v);
      if (rq_finite(v) && (key & digits) == prefix) atomicAdd(&l_hist[wave][(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t < 256) {
      unsigned s = 0;
      for (int w = 0; w < RQ_WAVES; ++w) s += l_hist[w][t];
      l_hist[0][t] = s;
    }
    __syncthreads();
    if (t == 0) {
      const unsigned k = l_sel[1];
      unsigned below = 0;
      int b = 0;
      for (; b < 255; ++b) {
        const unsigned h = l_hist[0][b];
        if (below + h > k) break;
        below += h;
      }
      l_sel[0] = prefix | ((unsigned)b << shift);
      l_sel[1] = k - below;
      l_sel[2] = l_hist[0][b];
    }
    __syncthreads();
    digits |= 255u << shift;
  }
  // the next order statistic: the same value while copies of it remain, else the smallest key above it
  const unsigned key_lo = l_sel[0];
  unsigned above = 0xffffffffu;
  for (int64_t i = t; i < N; i += RQ_THREADS) {
    const float v = x[i];
    const unsigned key = rq_key(v);
    if (rq_finite(v) && key > key_lo && key < above) above = key;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = (unsigned)__shfl_down((int)above, off, 64);
    above = o < above ? o : above;
  }
  if (lane == 0) l_red[wave] = above;
  __syncthreads();
  if (t == 0) {
    for (int w = 0; w < RQ_WAVES; ++w) above = l_red[w] < above ? l_red[w] : above;
    const double pos = fmin(fmax(q * (double)(M - 1), 0.0), (double)(M - 1));
    const double frac = pos - floor(pos);
    const double lo = (double)rq_value(key_lo);
    double hi = lo;
    if (frac > 0.0 && l_sel[1] + 1 >= l_sel[2] && above != 0xffffffffu) hi = (double)rq_value(above);
    *out = (float)(lo + (hi - lo) * frac);
  }
}

extern "C" int mnr_quantile(int64_t N, const float* x, double q, float* out, void* stream) {
  MNR_CHECK_ARG(N >= 1 && N < (1ll << 31) && x && out, "mnr_quantile: needs 1 <= N < 2^31 values and an output");
  MNR_CHECK_ARG(q >= 0.0 && q <= 1.0, "mnr_quantile: q = %g is outside [0, 1]", q);
  hipLaunchKernelGGL(quantile_kernel, dim3(1), dim3(RQ_THREADS), 0, (hipStream_t)stream, N, x, q, out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
