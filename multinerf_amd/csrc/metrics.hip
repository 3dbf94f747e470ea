// Evaluation metrics on device (gfx950): SSIM, the sums behind PSNR, and the Gram form of the colour correction.
//
// Replaces what the reference's eval.py:118-146 does per test image on the host: image.color_correct (image.py:81-124),
// the 8-bit quantisation and border crop, and MetricHarness (image.py:127-141: the mse and dm_pix.ssim).  The rendering
// and the ground truth are device tensors already; only scalars (and, per colour-correction iteration, three 10 x 10
// systems) go to the host.
//
// Every sum here is taken the same way: a thread adds its elements in a fixed order, a workgroup adds its threads by a
// tree in LDS, the workgroup's total goes to a `partials` array, and a second one-workgroup launch adds the partials in
// index order.  All in float64, no floating-point atomics: the result depends on the problem size only, and two runs
// agree bit for bit.
//
// SSIM: one workgroup per 32 x 16 tile of the SSIM map and channel.  The tile plus its (f - 1) halo of both images is
// staged in LDS once (float32, as given); the horizontal pass writes the five moment maps (a, b, a a, b b, a b) back to
// LDS in float64; the vertical pass and the SSIM expression stay in registers, two map elements per thread.  The window
// sums are float64 because sigma = filt(a a) - mu^2 cancels: in float32 its error (1e-7) is not small against
// c2 = 9e-4, and the scripts print the mean to four decimals.
//
// Colour correction: the reference solves lstsq([pixels, 10], b) for three channels, five times.  Its normal equations
// need sum f f^T (55 distinct entries) and sum f b (10) over the unmasked rows: 65 float64 accumulators per thread and
// channel, blockIdx.y = channel.  The host solves the 10 x 10 systems; mnr_cc_apply forms clip(A warp, 0, 1).
#include "common.h"

#define MT_THREADS 256
#define MT_MAX_BLOCKS 1024

// tree sum of one double per thread over the workgroup; the total is in red[0] after it (all threads must call)
__device__ __forceinline__ void mt_block_sum(double v, double* red, int t) {
  red[t] = v;
  __syncthreads();
  for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
}

// second stage: out[0] = (partials[0] + partials[1] + ...) / divisor, one workgroup, fixed order
__global__ __launch_bounds__(MT_THREADS) void sum_partials_kernel(const double* __restrict__ partials, int n, double divisor,
                                                                 double* out) {
  __shared__ double l_red[MT_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += MT_THREADS) s += partials[i];
  mt_block_sum(s, l_red, t);
  if (t == 0) out[0] = l_red[0] / divisor;
}

// ---------------------------------------------------------------------------
// SSIM

#define SS_TW 32
#define SS_TH 16
#define SS_ROWS (SS_TH / (MT_THREADS / SS_TW))             // map rows per thread: 2
#define SS_HW (SS_TW + MNR_SSIM_MAX_FILTER - 1)
#define SS_HH (SS_TH + MNR_SSIM_MAX_FILTER - 1)

struct ssim_window {
  double w[MNR_SSIM_MAX_FILTER];
};

__global__ __launch_bounds__(MT_THREADS) void ssim_kernel(mnr_ssim_args a, ssim_window win, int Ho, int Wo) {
  __shared__ float l_a[SS_HH * SS_HW];
  __shared__ float l_b[SS_HH * SS_HW];
  __shared__ double l_m[5][SS_HH][SS_TW];
  __shared__ double l_red[MT_THREADS];
  const int t = threadIdx.x;
  const int fs = a.filter_size, hw = SS_TW + fs - 1, hh = SS_TH + fs - 1;
  const int ch = blockIdx.z, ox0 = blockIdx.x * SS_TW, oy0 = blockIdx.y * SS_TH;
  const int He = a.H - 2 * a.crop, We = a.W - 2 * a.crop;
  // the tile and its halo; positions past the (cropped) image read as 0 and only feed map elements that are not kept
  for (int i = t; i < hh * hw; i += MT_THREADS) {
    const int y = i / hw, x = i - y * hw;
    const int gy = oy0 + y, gx = ox0 + x;
    float va = 0.0f, vb = 0.0f;
    if (gy < He && gx < We) {
      const int64_t at = ((int64_t)(gy + a.crop) * a.W + (gx + a.crop)) * a.C + ch;
      va = a.a[at];
      vb = a.b[at];
    }
    l_a[y * SS_HW + x] = va;
    l_b[y * SS_HW + x] = vb;
  }
  __syncthreads();
  // horizontal pass: five moment maps, LDS to LDS
  for (int i = t; i < hh * SS_TW; i += MT_THREADS) {
    const int y = i / SS_TW, x = i - y * SS_TW;
    double s0 = 0.0, s1 = 0.0, s00 = 0.0, s11 = 0.0, s01 = 0.0;
    for (int k = 0; k < fs; ++k) {
      const double w = win.w[k];
      const double va = (double)l_a[y * SS_HW + x + k], vb = (double)l_b[y * SS_HW + x + k];
      s0 += w * va;
      s1 += w * vb;
      s00 += w * (va * va);
      s11 += w * (vb * vb);
      s01 += w * (va * vb);
    }
    l_m[0][y][x] = s0;
    l_m[1][y][x] = s1;
    l_m[2][y][x] = s00;
    l_m[3][y][x] = s11;
    l_m[4][y][x] = s01;
  }
  __syncthreads();
  // vertical pass in registers: this thread's SS_ROWS map elements of column tx
  const int tx = t & (SS_TW - 1), ty = (t / SS_TW) * SS_ROWS;
  double acc[SS_ROWS][5];
#pragma unroll
  for (int o = 0; o < SS_ROWS; ++o) {
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
  }
  for (int r = 0; r < SS_ROWS + fs - 1; ++r) {
    double v[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) v[m] = l_m[m][ty + r][tx];
#pragma unroll
    for (int o = 0; o < SS_ROWS; ++o) {
      const int k = r - o;
      if (k >= 0 && k < fs) {
        const double w = win.w[k];
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] += w * v[m];
      }
    }
  }
  const double c1 = (a.k1 * a.max_val) * (a.k1 * a.max_val), c2 = (a.k2 * a.max_val) * (a.k2 * a.max_val);
  const double eps = (double)MNR_F32_EPS * (double)MNR_F32_EPS;
  double sum = 0.0;
#pragma unroll
  for (int o = 0; o < SS_ROWS; ++o) {
    const int oy = oy0 + ty + o, ox = ox0 + tx;
    if (oy < Ho && ox < Wo) {
      const double mu0 = acc[o][0], mu1 = acc[o][1];
      const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
      const double sigma00 = fmax(eps, acc[o][2] - mu00), sigma11 = fmax(eps, acc[o][3] - mu11);
      double sigma01 = acc[o][4] - mu01;
      const double lim = fmin(sqrt(sigma00 * sigma11), fabs(sigma01));
      sigma01 = sigma01 > 0.0 ? lim : (sigma01 < 0.0 ? -lim : 0.0);
      const double numer = (2.0 * mu01 + c1) * (2.0 * sigma01 + c2);
      const double denom = (mu00 + mu11 + c1) * (sigma00 + sigma11 + c2);
      const double s = numer / denom;
      if (a.map) a.map[((int64_t)oy * Wo + ox) * a.C + ch] = (float)s;
      sum += s;
    }
  }
  mt_block_sum(sum, l_red, t);
  if (t == 0) a.partials[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = l_red[0];
}

static int ssim_check(int H, int W, int C, int crop, int fs) {
  MNR_CHECK_ARG(H > 0 && W > 0 && C > 0 && crop >= 0, "mnr_ssim: bad image shape [%d, %d, %d] or crop %d", H, W, C, crop);
  MNR_CHECK_ARG(fs >= 1 && (fs & 1), "mnr_ssim: filter_size %d must be odd", fs);
  MNR_CHECK_ARG(fs <= MNR_SSIM_MAX_FILTER, "mnr_ssim: filter_size %d exceeds the compiled limit of %d", fs, MNR_SSIM_MAX_FILTER);
  MNR_CHECK_ARG((int64_t)H - 2 * (int64_t)crop >= fs && (int64_t)W - 2 * (int64_t)crop >= fs,
                "mnr_ssim: a [%d, %d] image cropped by %d is smaller than the %d x %d window", H, W, crop, fs, fs);
  MNR_CHECK_ARG((int64_t)H * W * C < (1ll << 31) && C <= 65535, "mnr_ssim: image too large");
  MNR_CHECK_ARG(mnr_cdiv((int64_t)H - 2 * (int64_t)crop - fs + 1, SS_TH) <= 65535,
                "mnr_ssim: a cropped height of %lld rows exceeds the limit of %d", (long long)H - 2 * (long long)crop, 65535 * SS_TH);
  return MNR_OK;
}

extern "C" int mnr_ssim_partials(int H, int W, int C, int crop, int filter_size) {
  if (ssim_check(H, W, C, crop, filter_size) != MNR_OK) return 0;
  const int Ho = H - 2 * crop - filter_size + 1, Wo = W - 2 * crop - filter_size + 1;
  return mnr_cdiv(Wo, SS_TW) * mnr_cdiv(Ho, SS_TH) * C;
}

extern "C" int mnr_ssim(const mnr_ssim_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->a && a->b && a->partials && a->out, "mnr_ssim: needs two images, the partials workspace and an output");
  const int st = ssim_check(a->H, a->W, a->C, a->crop, a->filter_size);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(a->filter_sigma > 0.0 && a->max_val > 0.0, "mnr_ssim: filter_sigma %g and max_val %g must be positive", a->filter_sigma,
                a->max_val);
  const int fs = a->filter_size;
  const int Ho = a->H - 2 * a->crop - fs + 1, Wo = a->W - 2 * a->crop - fs + 1;
  ssim_window win;
  double total = 0.0;
  for (int k = 0; k < MNR_SSIM_MAX_FILTER; ++k) {
    const double x = ((double)k - (double)(fs / 2)) / a->filter_sigma;
    win.w[k] = k < fs ? exp(-0.5 * x * x) : 0.0;
    total += win.w[k];
  }
  for (int k = 0; k < MNR_SSIM_MAX_FILTER; ++k) win.w[k] /= total;
  const dim3 grid(mnr_cdiv(Wo, SS_TW), mnr_cdiv(Ho, SS_TH), a->C);
  hipLaunchKernelGGL(ssim_kernel, grid, dim3(MT_THREADS), 0, (hipStream_t)stream, *a, win, Ho, Wo);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, a->partials,
                     (int)(grid.x * grid.y * grid.z), (double)Ho * (double)Wo * (double)a->C, a->out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// sum of squared differences, with the 8-bit quantisation and the crop of eval.py:134-143

__global__ __launch_bounds__(MT_THREADS) void sqdiff_kernel(mnr_sqdiff_args a, int64_t n) {
  __shared__ double l_red[MT_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + t; i < n; i += (int64_t)gridDim.x * MT_THREADS) {
    const int64_t p = i / a.C;
    const int y = (int)(p / a.W), x = (int)(p - (int64_t)y * a.W);
    double va = a.a_f64 ? ((const double*)a.a)[i] : (double)((const float*)a.a)[i];
    if (a.quantize) va = rint(va * 255.0) / 255.0;                         // np.round: half to even
    if (a.q_out) a.q_out[i] = (float)va;
    if (y >= a.crop && y < a.H - a.crop && x >= a.crop && x < a.W - a.crop) {
      const double vb = a.b_f64 ? ((const double*)a.b)[i] : (double)((const float*)a.b)[i];
      const double d = va - vb;
      s += d * d;
    }
  }
  mt_block_sum(s, l_red, t);
  if (t == 0) a.partials[blockIdx.x] = l_red[0];
}

static int mt_blocks(int64_t n) {
  const int64_t b = (n + MT_THREADS - 1) / MT_THREADS;
  return (int)(b < MT_MAX_BLOCKS ? b : MT_MAX_BLOCKS);
}

extern "C" int mnr_image_sqdiff_partials(int64_t n) { return n > 0 ? mt_blocks(n) : 0; }

extern "C" int mnr_image_sqdiff(const mnr_sqdiff_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->a && a->b && a->partials && a->out, "mnr_image_sqdiff: needs two images, the partials workspace and an output");
  MNR_CHECK_ARG(a->H > 0 && a->W > 0 && a->C > 0 && a->crop >= 0 && (int64_t)a->H * a->W * a->C < (1ll << 31),
                "mnr_image_sqdiff: bad image shape [%d, %d, %d] or crop %d", a->H, a->W, a->C, a->crop);
  MNR_CHECK_ARG(a->H > 2 * a->crop && a->W > 2 * a->crop, "mnr_image_sqdiff: a [%d, %d] image cropped by %d is empty", a->H, a->W,
                a->crop);
  const int64_t n = (int64_t)a->H * a->W * a->C;
  const int blocks = mt_blocks(n);
  hipLaunchKernelGGL(sqdiff_kernel, dim3(blocks), dim3(MT_THREADS), 0, (hipStream_t)stream, *a, n);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(MT_THREADS), 0, (hipStream_t)stream, a->partials, blocks, 1.0, a->out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// colour correction

#define CC_F MNR_CC_FEATURES
#define CC_OUT MNR_CC_GRAM_OUT
#define CC_ROUND 13                                        // accumulators reduced per pass through LDS (65 = 5 x 13)
#define CC_MAX_BLOCKS 512                                  // per channel: two workgroups per CU, and a short second stage

__device__ __forceinline__ void cc_features(double r, double g, double b, double* f) {
  f[0] = r * r;                                            // image.py:98-102: c * img[:, c:], then img, then 1
  f[1] = r * g;
  f[2] = r * b;
  f[3] = g * g;
  f[4] = g * b;
  f[5] = b * b;
  f[6] = r;
  f[7] = g;
  f[8] = b;
  f[9] = 1.0;
}

__device__ __forceinline__ bool cc_unclipped(double z, double eps) { return z >= eps && z <= 1.0 - eps; }

__global__ __launch_bounds__(MT_THREADS) void cc_gram_kernel(mnr_cc_gram_args a) {
  __shared__ double l_red[CC_ROUND][MT_THREADS];
  __shared__ double l_red2[CC_ROUND][16];
  const int t = threadIdx.x, c = blockIdx.y;
  double acc[CC_OUT];
#pragma unroll
  for (int k = 0; k < CC_OUT; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * MT_THREADS + t; i < a.N; i += (int64_t)gridDim.x * MT_THREADS) {
    const double z = a.img[i * 3 + c], bref = a.ref[i * 3 + c];
    bool m0;
    if (a.write_mask0) {
      m0 = cc_unclipped(z, a.eps);
      a.mask0[i * 3 + c] = m0 ? 1 : 0;
    } else {
      m0 = a.mask0[i * 3 + c] != 0;
    }
    if (m0 && cc_unclipped(z, a.eps) && cc_unclipped(bref, a.eps)) {          // image.py:111
      double f[CC_F];
      cc_features(a.img[i * 3 + 0], a.img[i * 3 + 1], a.img[i * 3 + 2], f);
      int k = 0;
#pragma unroll
      for (int p = 0; p < CC_F; ++p) {
#pragma unroll
        for (int q = p; q < CC_F; ++q) acc[k++] += f[p] * f[q];
      }
#pragma unroll
      for (int p = 0; p < CC_F; ++p) acc[55 + p] += f[p] * bref;
    }
  }
  // the workgroup's 65 sums, 13 at a time: 16 threads per accumulator add 16 entries each, then one thread adds the 16
  double* part = a.partials + ((int64_t)blockIdx.x * 3 + c) * CC_OUT;
#pragma unroll
  for (int round = 0; round < CC_OUT / CC_ROUND; ++round) {
#pragma unroll
    for (int j = 0; j < CC_ROUND; ++j) l_red[j][t] = acc[round * CC_ROUND + j];
    __syncthreads();
    if (t < CC_ROUND * 16) {
      const int j = t >> 4, seg = t & 15;
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += l_red[j][seg * 16 + k];
      l_red2[j][seg] = s;
    }
    __syncthreads();
    if (t < CC_ROUND) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += l_red2[t][k];
      part[round * CC_ROUND + t] = s;
    }
    __syncthreads();
  }
}

// second stage: out[c][k] = sum over the workgroups.  One thread per (entry, fifth of the workgroups) adds its partials in
// index order (975 of 1024 threads: a single thread per entry would wait for one load after the other), then the five
// sums are added in order.
#define CC_FINAL_THREADS 1024
#define CC_FINAL_PARTS 5
__global__ __launch_bounds__(CC_FINAL_THREADS) void cc_gram_final_kernel(const double* __restrict__ partials, int blocks, double* out) {
  __shared__ double l_part[CC_FINAL_PARTS][3 * CC_OUT];
  const int t = threadIdx.x, part = t / (3 * CC_OUT), e = t - part * (3 * CC_OUT);
  if (part < CC_FINAL_PARTS) {
    const int chunk = (blocks + CC_FINAL_PARTS - 1) / CC_FINAL_PARTS;
    const int b0 = part * chunk, b1 = min(b0 + chunk, blocks);
    double s = 0.0;
#pragma unroll 8
    for (int b = b0; b < b1; ++b) s += partials[(int64_t)b * 3 * CC_OUT + e];
    l_part[part][e] = s;
  }
  __syncthreads();
  if (t < 3 * CC_OUT) {
    double s = 0.0;
    for (int p = 0; p < CC_FINAL_PARTS; ++p) s += l_part[p][t];
    out[t] = s;
  }
}

static int cc_blocks(int64_t N) {
  const int64_t b = (N + MT_THREADS - 1) / MT_THREADS;
  return (int)(b < CC_MAX_BLOCKS ? b : CC_MAX_BLOCKS);
}

extern "C" int mnr_cc_gram_partials(int64_t N) { return N > 0 && N < (1ll << 31) ? cc_blocks(N) * 3 * CC_OUT : 0; }

extern "C" int mnr_cc_gram(const mnr_cc_gram_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->img && a->ref && a->mask0 && a->partials && a->out,
                "mnr_cc_gram: needs img, ref, mask0, the partials workspace and an output");
  MNR_CHECK_ARG(a->N > 0 && a->N < (1ll << 31), "mnr_cc_gram: needs 1 <= N < 2^31 pixels");
  MNR_CHECK_ARG(a->eps >= 0.0 && a->eps < 0.5, "mnr_cc_gram: eps = %g is outside [0, 0.5)", a->eps);
  const int blocks = cc_blocks(a->N);
  hipLaunchKernelGGL(cc_gram_kernel, dim3(blocks, 3), dim3(MT_THREADS), 0, (hipStream_t)stream, *a);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_gram_final_kernel, dim3(1), dim3(CC_FINAL_THREADS), 0, (hipStream_t)stream, a->partials, blocks, a->out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

struct cc_warp {
  double w[CC_F][3];
};

__global__ __launch_bounds__(MT_THREADS) void cc_apply_kernel(int64_t N, const double* img, cc_warp warp, double* out) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i >= N) return;
  double f[CC_F];
  cc_features(img[i * 3 + 0], img[i * 3 + 1], img[i * 3 + 2], f);
  double o[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < CC_F; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] += f[k] * warp.w[k][c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[i * 3 + c] = fmin(fmax(o[c], 0.0), 1.0);     // image.py:121-122
}

extern "C" int mnr_cc_apply(int64_t N, const double* img, const double* warp, double* out, void* stream) {
  MNR_CHECK_ARG(N > 0 && N < (1ll << 31) && img && warp && out, "mnr_cc_apply: needs 1 <= N < 2^31 pixels, img, warp [10,3] and out");
  cc_warp w;
  for (int k = 0; k < CC_F; ++k) {
    for (int c = 0; c < 3; ++c) {
      MNR_CHECK_ARG(warp[k * 3 + c] - warp[k * 3 + c] == 0.0, "mnr_cc_apply: warp[%d][%d] is not finite", k, c);
      w.w[k][c] = warp[k * 3 + c];
    }
  }
  hipLaunchKernelGGL(cc_apply_kernel, dim3(mnr_cdiv(N, MT_THREADS)), dim3(MT_THREADS), 0, (hipStream_t)stream, N, img, w, out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
