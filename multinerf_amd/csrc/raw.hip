// RawNeRF data path on device (gfx950): what the reference's internal/raw_utils.py does per pixel.
//
//   mnr_raw_demosaic     load_raw_dataset:354-382 for a stack of Bayer mosaics: black / white level normalisation in
//                        float64 (one rounding to float32), bilinear_demosaic with its np.roll wrap-around in float32,
//                        and the area downsample of image.downsample fused (the full-resolution image is never written);
//   mnr_raw_postprocess  postprocess_raw: camera -> linear RGB, exposure, clip, sRGB curve, in float64;
//   mnr_quantile_f64     np.percentile of a float64 array: exact radix select over many workgroups;
//   mnr_affine_sums /    best_fit_affine / match_images_affine for axis = (0, 1).
//   mnr_affine_apply
//
// All of it is bound by memory.  The demosaic reads every mosaic value through the caches (a 4 x 4 window per 2 x 2 quad;
// neighbouring threads share 12 of its 16 values, so HBM sees each value about once; each is normalised once per thread) and writes 24 contiguous bytes per
// thread and row.  Sums are per-workgroup float64 partials added by a second one-workgroup launch in index order, the
// radix select merges per-workgroup LDS histograms with integer atomics: two runs agree bit for bit.
#include "common.h"

#define RW_THREADS 256

// ---------------------------------------------------------------------------
// demosaic

struct rw_mosaic {
  const void* m;                   // one image [H,W]
  int H, W, f32, norm;
  double black, den, scale;
};

// g(y, x) = m[y mod H, x mod W] for -2 <= y < H + 2 (one wrap), normalised in float64 and rounded once
__device__ __forceinline__ float rw_g(const rw_mosaic& s, int y, int x) {
  y = y < 0 ? y + s.H : (y >= s.H ? y - s.H : y);
  x = x < 0 ? x + s.W : (x >= s.W ? x - s.W : x);
  const int64_t at = (int64_t)y * s.W + x;
  const float v = s.f32 ? ((const float*)s.m)[at] : (float)((const uint16_t*)s.m)[at];
  if (!s.norm) return v;
  return (float)(((double)v - s.black) / s.den * s.scale);
}

// bilinear_demosaic (raw_utils.py:80-146) of pixel (y, x) with parities (py, px) in closed form, over a getter g(y, x) of
// the (wrapped) mosaic; every product is by a power of two
template <class G>
__device__ __forceinline__ void rw_demosaic_px(const G& g, int y, int x, int py, int px, float* rgb) {
  const int y0 = y - py, x0 = x - px, y1 = y + 1 - py, x1 = x + 1 - px;
  float r, gr, b;
  if (!py && !px) {
    r = g(y0, x0);
  } else if (!py) {
    r = .5f * (g(y0, x0) + g(y0, x0 + 2));
  } else if (!px) {
    r = .5f * (g(y0, x0) + g(y0 + 2, x0));
  } else {
    r = .5f * (.5f * (g(y0, x0) + g(y0, x0 + 2)) + .5f * (g(y0 + 2, x0) + g(y0 + 2, x0 + 2)));
  }
  if (py && px) {
    b = g(y1, x1);
  } else if (py) {
    b = .5f * (g(y1, x1) + g(y1, x1 - 2));
  } else if (px) {
    b = .5f * (g(y1, x1) + g(y1 - 2, x1));
  } else {
    b = .5f * (.5f * (g(y1, x1) + g(y1, x1 - 2)) + .5f * (g(y1 - 2, x1) + g(y1 - 2, x1 - 2)));
  }
  if (py != px) {
    gr = g(y, x);
  } else {
    gr = (((.25f * g(y, x + 1)) + .25f * g(y, x - 1)) + .25f * g(y + 1, x)) + .25f * g(y - 1, x);
  }
  rgb[0] = r;
  rgb[1] = gr;
  rgb[2] = b;
}

struct rw_demosaic_args {
  int H, W, f32, n;
  const void* mosaic;              // [N,H,W]
  const double* black;             // [N] or NULL
  const double* white;
  double scale;
  float* out;                      // [N, H/n, W/n, 3]
};

__device__ __forceinline__ rw_mosaic rw_image(const rw_demosaic_args& a, int img) {
  rw_mosaic s;
  const int64_t off = (int64_t)img * a.H * a.W;
  s.m = a.f32 ? (const void*)((const float*)a.mosaic + off) : (const void*)((const uint16_t*)a.mosaic + off);
  s.H = a.H;
  s.W = a.W;
  s.f32 = a.f32;
  s.norm = a.black != nullptr;
  s.black = s.norm ? a.black[img] : 0.0;
  s.den = s.norm ? a.white[img] - a.black[img] : 1.0;
  s.scale = a.scale;
  return s;
}

// n = 1: one thread per 2 x 2 quad, block (64, 4) quads; per row six floats = three 8-byte stores, contiguous over the wave
__global__ __launch_bounds__(RW_THREADS) void raw_demosaic_quad_kernel(rw_demosaic_args a) {
  const int qx = blockIdx.x * 64 + threadIdx.x, qy = blockIdx.y * 4 + threadIdx.y, img = blockIdx.z;
  if (qx >= a.W / 2 || qy >= a.H / 2) return;
  const rw_mosaic s = rw_image(a, img);
  float w[4][4];                                           // the quad and its one-pixel border: each value loaded and normalised once
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) w[r][c] = rw_g(s, 2 * qy - 1 + r, 2 * qx - 1 + c);
  }
  const auto window = [&w](int y, int x) { return w[y + 1][x + 1]; };      // coordinates relative to the quad
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    float v[6];
    rw_demosaic_px(window, dy, 0, dy, 0, v);
    rw_demosaic_px(window, dy, 1, dy, 1, v + 3);
    f32x2* o = (f32x2*)(a.out + (((int64_t)img * a.H + (2 * qy + dy)) * a.W + 2 * qx) * 3);
    f32x2 p0 = {v[0], v[1]}, p1 = {v[2], v[3]}, p2 = {v[4], v[5]};
    o[0] = p0;
    o[1] = p1;
    o[2] = p2;
  }
}

// n > 1: one thread per output pixel; the n x n demosaicked float32 values are added in float64, row by row, and the
// mean is rounded once (image.downsample)
__global__ __launch_bounds__(RW_THREADS) void raw_demosaic_down_kernel(rw_demosaic_args a) {
  const int Wo = a.W / a.n, Ho = a.H / a.n;
  const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y, img = blockIdx.z;
  if (ox >= Wo || oy >= Ho) return;
  const rw_mosaic s = rw_image(a, img);
  const auto mosaic = [&s](int y, int x) { return rw_g(s, y, x); };
  double acc[3] = {0.0, 0.0, 0.0};
  for (int dy = 0; dy < a.n; ++dy) {
    for (int dx = 0; dx < a.n; ++dx) {
      float v[3];
      const int y = oy * a.n + dy, x = ox * a.n + dx;
      rw_demosaic_px(mosaic, y, x, y & 1, x & 1, v);
      acc[0] += (double)v[0];
      acc[1] += (double)v[1];
      acc[2] += (double)v[2];
    }
  }
  const double cnt = (double)a.n * (double)a.n;
  float* o = a.out + (((int64_t)img * Ho + oy) * Wo + ox) * 3;
  o[0] = (float)(acc[0] / cnt);
  o[1] = (float)(acc[1] / cnt);
  o[2] = (float)(acc[2] / cnt);
}

extern "C" int mnr_raw_demosaic(int N, int H, int W, int dtype, const void* mosaic, const double* black, const double* white,
                                double scale, int n_downsample, float* out, void* stream) {
  MNR_CHECK_ARG(mosaic && out, "mnr_raw_demosaic: needs a mosaic and an output");
  MNR_CHECK_ARG(N >= 1 && N <= 65535, "mnr_raw_demosaic: needs 1 <= N <= 65535 images, got %d", N);
  MNR_CHECK_ARG(H >= 2 && W >= 2 && !(H & 1) && !(W & 1), "mnr_raw_demosaic: a Bayer mosaic has even height and width, got [%d, %d]", H, W);
  MNR_CHECK_ARG(dtype == MNR_RAW_U16 || dtype == MNR_RAW_F32, "mnr_raw_demosaic: dtype %d is neither MNR_RAW_U16 nor MNR_RAW_F32", dtype);
  MNR_CHECK_ARG((black == nullptr) == (white == nullptr), "mnr_raw_demosaic: black and white levels go together");
  MNR_CHECK_ARG(n_downsample >= 1 && H % n_downsample == 0 && W % n_downsample == 0,
                "mnr_raw_demosaic: n_downsample = %d must divide the image shape [%d, %d]", n_downsample, H, W);
  MNR_CHECK_ARG((int64_t)H * W < (1ll << 31), "mnr_raw_demosaic: image too large");
  MNR_CHECK_ARG(((size_t)out & 7) == 0, "mnr_raw_demosaic: out must be aligned to 8 bytes (it is written in pairs of floats)");
  const int Ho = H / n_downsample, Wo = W / n_downsample;
  const int ux = n_downsample == 1 ? W / 2 : Wo, uy = n_downsample == 1 ? H / 2 : Ho;      // threads needed per image
  MNR_CHECK_ARG(mnr_cdiv(uy, 4) <= 65535, "mnr_raw_demosaic: %d rows exceed the grid limit", H);
  rw_demosaic_args a;
  a.H = H;
  a.W = W;
  a.f32 = dtype == MNR_RAW_F32;
  a.n = n_downsample;
  a.mosaic = mosaic;
  a.black = black;
  a.white = white;
  a.scale = scale;
  a.out = out;
  const dim3 grid(mnr_cdiv(ux, 64), mnr_cdiv(uy, 4), N), block(64, 4);
  if (n_downsample == 1) {
    hipLaunchKernelGGL(raw_demosaic_quad_kernel, grid, block, 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(raw_demosaic_down_kernel, grid, block, 0, (hipStream_t)stream, a);
  }
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// post-processing

__global__ __launch_bounds__(RW_THREADS) void raw_postprocess_kernel(mnr_raw_post_args a) {
  const int64_t i = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x;
  if (i >= a.P) return;
  double c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = a.raw_f64 ? ((const double*)a.raw)[i * 3 + k] : (double)((const float*)a.raw)[i * 3 + k];
  double lin[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) lin[k] = (c[0] * a.camtorgb[k * 3 + 0] + c[1] * a.camtorgb[k * 3 + 1]) + c[2] * a.camtorgb[k * 3 + 2];
  if (a.linear_only) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_f64[i * 3 + k] = lin[k];
    return;
  }
  const double exposure = a.exposure_dev ? a.exposure_dev[0] : a.exposure;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double q = lin[k] / exposure;
    const double z = q != q ? q : fmin(fmax(q, 0.0), 1.0);                 // np.clip keeps NaN
    const double s0 = 323.0 / 25.0 * z;                                     // image.py:42-48
    const double s1 = (211.0 * pow(fmax((double)MNR_F32_EPS, z), 5.0 / 12.0) - 11.0) / 200.0;
    const double srgb = z != z ? z : (z <= 0.0031308 ? s0 : s1);
    if (a.out_f64) a.out_f64[i * 3 + k] = srgb;
    if (a.out_f32) a.out_f32[i * 3 + k] = (float)srgb;
    if (a.out_u8) {                                                         // utils.save_img_u8: nan_to_num, clip, * 255, truncate
      const double u = srgb != srgb ? 0.0 : fmin(fmax(srgb, 0.0), 1.0);
      a.out_u8[i * 3 + k] = (unsigned char)(int)(u * 255.0);
    }
  }
}

extern "C" int mnr_raw_postprocess(const mnr_raw_post_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->raw, "mnr_raw_postprocess: needs an input image");
  MNR_CHECK_ARG(a->P >= 1 && a->P < (1ll << 31), "mnr_raw_postprocess: needs 1 <= P < 2^31 pixels");
  if (a->linear_only) {
    MNR_CHECK_ARG(a->out_f64 && !a->out_f32 && !a->out_u8, "mnr_raw_postprocess: the linear mode writes out_f64 only");
  } else {
    MNR_CHECK_ARG(a->out_f64 || a->out_f32 || a->out_u8, "mnr_raw_postprocess: needs at least one output");
    MNR_CHECK_ARG(a->exposure_dev || a->exposure == a->exposure, "mnr_raw_postprocess: the exposure is NaN");
  }
  for (int k = 0; k < 9; ++k) MNR_CHECK_ARG(a->camtorgb[k] - a->camtorgb[k] == 0.0, "mnr_raw_postprocess: camtorgb[%d] is not finite", k);
  hipLaunchKernelGGL(raw_postprocess_kernel, dim3(mnr_cdiv(a->P, RW_THREADS)), dim3(RW_THREADS), 0, (hipStream_t)stream, *a);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// np.percentile of float64 values: most-significant-digit radix select on the 64-bit patterns, 8 bits a pass, many
// workgroups.  Keys are the bit patterns in their total order (sign set for positive values, all bits flipped for
// negative ones).  Pass p histograms digit p of the values whose higher digits equal the prefix chosen so far: one LDS
// histogram per wave, merged into the pass's global histogram by integer atomics (exact, order-independent).  The
// selection is no launch of its own: every workgroup of pass p derives it from pass p - 1's finished histogram and the
// state pass p - 1 left, and workgroup 0 records the state for the next pass.
//
// workspace (uint32 words): hist[8][256] | state[9][QS_WORDS] | keys above per workgroup [QF_MAX_BLOCKS][2]

#define QF_WAVES (RW_THREADS / 64)
#define QF_PASSES 8
#define QF_MAX_BLOCKS 2048
#define QS_WORDS 8                  // prefix lo, prefix hi, rank, bin count, finite count M, pad
#define QF_HIST_WORDS (QF_PASSES * 256)
#define QF_STATE_OFF QF_HIST_WORDS
#define QF_ABOVE_OFF (QF_STATE_OFF + (QF_PASSES + 1) * QS_WORDS)
#define QF_WORDS (QF_ABOVE_OFF + 2 * QF_MAX_BLOCKS)

__device__ __forceinline__ uint64_t qf_key(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double qf_value(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
__device__ __forceinline__ bool qf_finite(double v) {
  return (__builtin_bit_cast(uint64_t, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

struct qf_state {
  uint64_t prefix;                 // the digits chosen so far, in place
  unsigned rank, count, M;         // rank of the wanted value inside the chosen bin; the bin's size; finite values in all
};

__device__ __forceinline__ double qf_position(double p, unsigned M) {
  const double pos = (double)(M - 1) * (p / 100.0);        // numpy: (n - 1) * quantile
  return fmin(fmax(pos, 0.0), (double)(M - 1));
}

// The state after passes 0 .. pass - 1 (pass >= 1), from hist[pass - 1] and state[pass - 1]; all threads must call.
// l_scan: 256 words of LDS, l_sel: QS_WORDS words.
__device__ __forceinline__ qf_state qf_resolve(const unsigned* ws, int pass, double p, unsigned* l_scan, unsigned* l_sel, unsigned* ws_out) {
  const int t = threadIdx.x;
  const unsigned h = ws[(pass - 1) * 256 + t];
  l_scan[t] = h;
  __syncthreads();
  unsigned inc = h;                                        // inclusive prefix sum over the 256 bins (Hillis-Steele)
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned add = t >= off ? l_scan[t - off] : 0u;
    __syncthreads();
    inc += add;
    l_scan[t] = inc;
    __syncthreads();
  }
  qf_state prev;
  if (pass == 1) {
    prev.prefix = 0;
    prev.M = l_scan[255];
    prev.rank = prev.M ? (unsigned)floor(qf_position(p, prev.M)) : 0u;
    prev.count = prev.M;
  } else {
    const unsigned* st = ws + QF_STATE_OFF + (pass - 1) * QS_WORDS;
    prev.prefix = ((uint64_t)st[1] << 32) | st[0];
    prev.rank = st[2];
    prev.count = st[3];
    prev.M = st[4];
  }
  if (t == 0) {
    l_sel[0] = l_sel[1] = l_sel[2] = l_sel[3] = 0;
    l_sel[4] = prev.M;
  }
  __syncthreads();
  if (prev.M != 0 && inc > prev.rank && inc - h <= prev.rank) {           // exactly one bin holds the rank
    const uint64_t prefix = prev.prefix | ((uint64_t)t << (56 - 8 * (pass - 1)));
    l_sel[0] = (unsigned)prefix;
    l_sel[1] = (unsigned)(prefix >> 32);
    l_sel[2] = prev.rank - (inc - h);
    l_sel[3] = h;
  }
  __syncthreads();
  qf_state s;
  s.prefix = ((uint64_t)l_sel[1] << 32) | l_sel[0];
  s.rank = l_sel[2];
  s.count = l_sel[3];
  s.M = l_sel[4];
  if (ws_out && blockIdx.x == 0 && t < 5) ws_out[QF_STATE_OFF + pass * QS_WORDS + t] = l_sel[t];
  return s;
}

__global__ __launch_bounds__(RW_THREADS) void quantile_f64_zero_kernel(unsigned* ws) {
  for (int i = threadIdx.x; i < QF_ABOVE_OFF; i += RW_THREADS) ws[i] = 0;
}

__global__ __launch_bounds__(RW_THREADS) void quantile_f64_hist_kernel(int64_t N, const double* __restrict__ x, double p, int pass,
                                                                      unsigned* ws) {
  __shared__ unsigned l_hist[QF_WAVES][256];
  __shared__ unsigned l_scan[256];
  __shared__ unsigned l_sel[QS_WORDS];
  const int t = threadIdx.x, wave = t >> 6;
  qf_state s;
  s.prefix = 0;
  s.M = 1;
  if (pass > 0) s = qf_resolve(ws, pass, p, l_scan, l_sel, ws);
  if (s.M == 0) return;                                    // no finite value (uniform over the grid)
  for (int b = t; b < QF_WAVES * 256; b += RW_THREADS) (&l_hist[0][0])[b] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const uint64_t digits = pass == 0 ? 0ull : (~0ull << (shift + 8));
  for (int64_t i = (int64_t)blockIdx.x * RW_THREADS + t; i < N; i += (int64_t)gridDim.x * RW_THREADS) {
    const double v = x[i];
    const uint64_t key = qf_key(v);
    if (qf_finite(v) && (key & digits) == s.prefix) atomicAdd(&l_hist[wave][(unsigned)(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  unsigned sum = 0;
#pragma unroll
  for (int w = 0; w < QF_WAVES; ++w) sum += l_hist[w][t];
  if (sum) atomicAdd(&ws[pass * 256 + t], sum);
}

// the smallest key above the selected one, per workgroup (the next order statistic when no copy of the selected one is left)
__global__ __launch_bounds__(RW_THREADS) void quantile_f64_above_kernel(int64_t N, const double* __restrict__ x, double p, unsigned* ws) {
  __shared__ unsigned l_scan[256];
  __shared__ unsigned l_sel[QS_WORDS];
  __shared__ uint64_t l_min[RW_THREADS];
  const int t = threadIdx.x;
  const qf_state s = qf_resolve(ws, QF_PASSES, p, l_scan, l_sel, ws);
  uint64_t above = ~0ull;
  if (s.M != 0) {
    for (int64_t i = (int64_t)blockIdx.x * RW_THREADS + t; i < N; i += (int64_t)gridDim.x * RW_THREADS) {
      const double v = x[i];
      const uint64_t key = qf_key(v);
      if (qf_finite(v) && key > s.prefix && key < above) above = key;
    }
  }
  l_min[t] = above;
  __syncthreads();
  for (int st = RW_THREADS / 2; st > 0; st >>= 1) {
    if (t < st) l_min[t] = l_min[t + st] < l_min[t] ? l_min[t + st] : l_min[t];
    __syncthreads();
  }
  if (t == 0) {
    ws[QF_ABOVE_OFF + 2 * blockIdx.x] = (unsigned)l_min[0];
    ws[QF_ABOVE_OFF + 2 * blockIdx.x + 1] = (unsigned)(l_min[0] >> 32);
  }
}

__global__ __launch_bounds__(RW_THREADS) void quantile_f64_final_kernel(double p, int blocks, const unsigned* ws, double* out) {
  __shared__ uint64_t l_min[RW_THREADS];
  const int t = threadIdx.x;
  uint64_t above = ~0ull;
  for (int b = t; b < blocks; b += RW_THREADS) {
    const uint64_t k = ((uint64_t)ws[QF_ABOVE_OFF + 2 * b + 1] << 32) | ws[QF_ABOVE_OFF + 2 * b];
    above = k < above ? k : above;
  }
  l_min[t] = above;
  __syncthreads();
  for (int st = RW_THREADS / 2; st > 0; st >>= 1) {
    if (t < st) l_min[t] = l_min[t + st] < l_min[t] ? l_min[t + st] : l_min[t];
    __syncthreads();
  }
  if (t == 0) {
    const unsigned* st = ws + QF_STATE_OFF + QF_PASSES * QS_WORDS;
    const uint64_t key_lo = ((uint64_t)st[1] << 32) | st[0];
    const unsigned rank = st[2], count = st[3], M = st[4];
    if (M == 0) {
      out[0] = __builtin_bit_cast(double, 0x7ff8000000000000ull);
      return;
    }
    const double pos = qf_position(p, M);
    const double frac = pos - floor(pos);
    const double a = qf_value(key_lo);
    double b = a;                                          // the value at floor(pos) + 1, where that exists
    if ((unsigned)floor(pos) + 1 < M && rank + 1 >= count && l_min[0] != ~0ull) b = qf_value(l_min[0]);
    const double d = b - a;                                // numpy's _lerp
    out[0] = frac >= 0.5 ? b - d * (1.0 - frac) : a + d * frac;
  }
}

static int qf_blocks(int64_t N) {
  const int64_t b = (N + RW_THREADS * 8 - 1) / (RW_THREADS * 8);           // eight values per thread and pass at least
  return (int)(b < 1 ? 1 : (b < QF_MAX_BLOCKS ? b : QF_MAX_BLOCKS));
}

extern "C" int64_t mnr_quantile_f64_workspace(int64_t N) { return N >= 1 && N < (1ll << 31) ? (int64_t)QF_WORDS * 4 : 0; }

extern "C" int mnr_quantile_f64(int64_t N, const double* x, double p, void* workspace, double* out, void* stream) {
  MNR_CHECK_ARG(N >= 1 && N < (1ll << 31) && x && workspace && out,
                "mnr_quantile_f64: needs 1 <= N < 2^31 values, the workspace of mnr_quantile_f64_workspace(N) bytes and an output");
  MNR_CHECK_ARG(p >= 0.0 && p <= 100.0, "mnr_quantile_f64: p = %g is outside [0, 100]", p);
  unsigned* ws = (unsigned*)workspace;
  const int blocks = qf_blocks(N);
  hipLaunchKernelGGL(quantile_f64_zero_kernel, dim3(1), dim3(RW_THREADS), 0, (hipStream_t)stream, ws);
  MNR_CHECK_LAUNCH();
  for (int pass = 0; pass < QF_PASSES; ++pass) {
    hipLaunchKernelGGL(quantile_f64_hist_kernel, dim3(blocks), dim3(RW_THREADS), 0, (hipStream_t)stream, N, x, p, pass, ws);
    MNR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(quantile_f64_above_kernel, dim3(blocks), dim3(RW_THREADS), 0, (hipStream_t)stream, N, x, p, ws);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(quantile_f64_final_kernel, dim3(1), dim3(RW_THREADS), 0, (hipStream_t)stream, p, blocks, ws, out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// affine match

#define AF_SUMS 12                  // per channel: gt, est, gt est, gt gt
#define AF_MAX_BLOCKS 1024

__global__ __launch_bounds__(RW_THREADS) void affine_sums_kernel(int64_t P, const double* __restrict__ est, const double* __restrict__ gt,
                                                                double* partials) {
  __shared__ double l_red[AF_SUMS][RW_THREADS];
  __shared__ double l_red2[AF_SUMS][16];
  const int t = threadIdx.x;
  double acc[AF_SUMS];
#pragma unroll
  for (int k = 0; k < AF_SUMS; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * RW_THREADS + t; i < P; i += (int64_t)gridDim.x * RW_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double g = gt[i * 3 + c], e = est[i * 3 + c];
      acc[0 * 3 + c] += g;
      acc[1 * 3 + c] += e;
      acc[2 * 3 + c] += g * e;
      acc[3 * 3 + c] += g * g;
    }
  }
  // the workgroup's 12 sums: 16 threads per sum add 16 entries each in order, then one thread adds the 16
#pragma unroll
  for (int k = 0; k < AF_SUMS; ++k) l_red[k][t] = acc[k];
  __syncthreads();
  if (t < AF_SUMS * 16) {
    const int k = t >> 4, seg = t & 15;
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += l_red[k][seg * 16 + j];
    l_red2[k][seg] = s;
  }
  __syncthreads();
  if (t < AF_SUMS) {
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += l_red2[t][j];
    partials[(int64_t)blockIdx.x * AF_SUMS + t] = s;
  }
}

// second stage, one workgroup: 16 threads per sum add a sixteenth of the workgroups' partials each, in index order, then one
// thread adds the 16
__global__ __launch_bounds__(RW_THREADS) void affine_sums_final_kernel(const double* __restrict__ partials, int blocks, double* out) {
  __shared__ double l_red2[AF_SUMS][16];
  const int t = threadIdx.x;
  if (t < AF_SUMS * 16) {
    const int k = t >> 4, seg = t & 15;
    const int chunk = (blocks + 15) / 16;
    const int b0 = seg * chunk, b1 = min(b0 + chunk, blocks);
    double s = 0.0;
    for (int b = b0; b < b1; ++b) s += partials[(int64_t)b * AF_SUMS + k];
    l_red2[k][seg] = s;
  }
  __syncthreads();
  if (t < AF_SUMS) {
    double s = 0.0;
    for (int j = 0; j < 16; ++j) s += l_red2[t][j];
    out[t] = s;
  }
}

static int af_blocks(int64_t P) {
  const int64_t b = (P + RW_THREADS - 1) / RW_THREADS;
  return (int)(b < AF_MAX_BLOCKS ? b : AF_MAX_BLOCKS);
}

extern "C" int mnr_affine_sums_partials(int64_t P) { return P >= 1 ? af_blocks(P) * AF_SUMS : 0; }

extern "C" int mnr_affine_sums(int64_t P, const double* est, const double* gt, double* partials, double* out, void* stream) {
  MNR_CHECK_ARG(P >= 1 && P < (1ll << 31) && est && gt && partials && out, "mnr_affine_sums: needs 1 <= P < 2^31 pixels, est, gt, the partials workspace and an output");
  const int blocks = af_blocks(P);
  hipLaunchKernelGGL(affine_sums_kernel, dim3(blocks), dim3(RW_THREADS), 0, (hipStream_t)stream, P, est, gt, partials);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(affine_sums_final_kernel, dim3(1), dim3(RW_THREADS), 0, (hipStream_t)stream, partials, blocks, out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

struct af_coeffs {
  double a[3], b[3];
};

__global__ __launch_bounds__(RW_THREADS) void affine_apply_kernel(int64_t n, const double* est, af_coeffs k, double* out) {
  const int64_t i = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % 3);
  out[i] = (est[i] - k.b[c]) / k.a[c];
}

extern "C" int mnr_affine_apply(int64_t P, const double* est, const double* a, const double* b, double* out, void* stream) {
  MNR_CHECK_ARG(P >= 1 && P < (1ll << 31) && est && a && b && out, "mnr_affine_apply: needs 1 <= P < 2^31 pixels, est, a[3], b[3] and out");
  af_coeffs k;
  for (int c = 0; c < 3; ++c) {
    k.a[c] = a[c];
    k.b[c] = b[c];
  }
  hipLaunchKernelGGL(affine_apply_kernel, dim3(mnr_cdiv(P * 3, RW_THREADS)), dim3(RW_THREADS), 0, (hipStream_t)stream, P * 3, est, k, out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
