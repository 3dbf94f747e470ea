// Visualisation of a rendering on device (gfx950): the per-pixel work of the reference's internal/vis.py and of
// render.py:86-93, on the rendering where it already lies.
//
//   mnr_weighted_percentile  vis.weighted_percentile (vis.py:22-30) on data the caller has ordered
//   mnr_vis_cmap             the per-pixel part of vis.visualize_cmap (vis.py:85-106), optionally matted, optionally 8-bit
//   mnr_vis_matte            vis.matte (vis.py:39-45) behind a small pre-op (normals, roughness, visualize_coord_mod)
//
// Arithmetic is float64 on the float32 inputs, rounded once at the store; FP contraction is off so that the operation
// order written here is the one executed (the mod of visualize_coord_mod and the LUT index are discontinuous).
//
// Weighted percentile.  The running sum of the weights is defined, once, as a fixed three-level sum, and every kernel
// that needs a value of it recomputes it by that definition, so it is one non-decreasing array whatever the launch:
//   the N sorted elements are cut into nseg segments of seg_len, a segment into WP_THREADS chunks of `chunk` consecutive
//   elements;  r   = sum of the chunk's weights up to the element, in index order
//              Q_t = c_0 + c_1 + ... + c_(t-1), the chunk totals of the segment added in index order
//              P_s = S_0 + S_1 + ... + S_(s-1), the segment totals (S = Q_WP_THREADS) added in index order
//              acc[i] = P_s + (Q_t + r).
//   The last element of a chunk then has acc = P_s + Q_(t+1), the start value of the next chunk, and the last of a segment
//   P_(s+1): the array is continuous across the cuts, and (for weights >= 0) non-decreasing, because fl(a + b) is monotone
//   in b.  No floating-point atomics: two runs agree bit for bit.
//   wp_segment_kernel writes the S, wp_scan_kernel the P; wp_interp_kernel, one workgroup per (segment, percentile),
//   leaves at once unless T = p acc[N-1] / 100 falls into its segment, and otherwise finds the one element i with
//   acc[i-1] <= T < acc[i]: j = i - 1 is the last index with acc[j] <= T, which is where np.interp(T, acc, x) interpolates.
#include "common.h"

#pragma clang fp contract(off)

#define WP_THREADS 256
#define WP_MAX_SEGS 1024
#define WP_SEG_MIN 1024                                  // elements of a segment when N allows more than one

struct wp_plan {
  int64_t N, NW, seg_len;
  int nseg, chunk;
};

static wp_plan wp_make_plan(int64_t N, int64_t NW) {
  wp_plan p;
  p.N = N;
  p.NW = NW;
  int64_t nseg = (N + WP_SEG_MIN - 1) / WP_SEG_MIN;
  if (nseg > WP_MAX_SEGS) nseg = WP_MAX_SEGS;
  if (nseg < 1) nseg = 1;
  const int64_t per = (N + nseg - 1) / nseg;
  p.chunk = (int)((per + WP_THREADS - 1) / WP_THREADS);
  p.seg_len = (int64_t)p.chunk * WP_THREADS;
  p.nseg = (int)((N + p.seg_len - 1) / p.seg_len);
  return p;
}

__device__ __forceinline__ double wp_weight(const wp_plan& pl, const int64_t* __restrict__ order, const float* __restrict__ w,
                                            int64_t i) {
  int64_t k = order[i];
  k = k < 0 ? 0 : (k >= pl.NW ? pl.NW - 1 : k);           // a gather that clamps, as jax documents for x[indices]
  return (double)w[k];
}

// the chunk totals of this workgroup's segment into l_q, then Q (exclusive, in index order) in their place; l_q[WP_THREADS] = S
__device__ __forceinline__ void wp_segment_scan(const wp_plan& pl, const int64_t* __restrict__ order, const float* __restrict__ w,
                                                int seg, double* l_q) {
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)seg * pl.seg_len + (int64_t)t * pl.chunk;
  double c = 0.0;
  for (int k = 0; k < pl.chunk; ++k) {
    const int64_t i = i0 + k;
    if (i < pl.N) c += wp_weight(pl, order, w, i);
  }
  l_q[t] = c;
  __syncthreads();
  if (t == 0) {
    double q = 0.0;
    for (int k = 0; k < WP_THREADS; ++k) {
      const double ck = l_q[k];
      l_q[k] = q;
      q += ck;
    }
    l_q[WP_THREADS] = q;
  }
  __syncthreads();
}

__global__ __launch_bounds__(WP_THREADS) void wp_segment_kernel(wp_plan pl, const int64_t* __restrict__ order,
                                                              const float* __restrict__ w, double* __restrict__ seg_total) {
  __shared__ double l_q[WP_THREADS + 1];
  wp_segment_scan(pl, order, w, blockIdx.x, l_q);
  if (threadIdx.x == 0) seg_total[blockIdx.x] = l_q[WP_THREADS];
}

// P[0] = 0, P[s + 1] = P[s] + S[s]: one workgroup, the totals staged in LDS, one thread adds them in index order
__global__ __launch_bounds__(WP_THREADS) void wp_scan_kernel(int nseg, const double* __restrict__ seg_total, double* __restrict__ P) {
  __shared__ double l_s[WP_MAX_SEGS];
  for (int i = threadIdx.x; i < nseg; i += WP_THREADS) l_s[i] = seg_total[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = 0.0;
    P[0] = p;
    for (int s = 0; s < nseg; ++s) {
      p += l_s[s];
      P[s + 1] = p;
    }
  }
}

struct wp_ps {
  double p[MNR_VIS_MAX_PERCENTILES];
};

__global__ __launch_bounds__(WP_THREADS) void wp_interp_kernel(wp_plan pl, const float* __restrict__ x, const int64_t* __restrict__ order,
                                                             const float* __restrict__ w, const double* __restrict__ P, wp_ps ps,
                                                             float* __restrict__ out) {
  __shared__ double l_q[WP_THREADS + 1];
  const int seg = blockIdx.x, ip = blockIdx.y, t = threadIdx.x;
  const double total = P[pl.nseg];
  const double T = ps.p[ip] * (total / 100.0);             // vis.py:30
  if (!(T < total)) {                                      // T >= acc[-1] (all-zero weights included): x[-1]
    if (seg == 0 && t == 0) out[ip] = x[pl.N - 1];
    return;
  }
  const double p0 = P[seg], p1 = P[seg + 1];
  if (!(p0 <= T && T < p1)) return;                        // (the same for every thread of the workgroup)
  wp_segment_scan(pl, order, w, seg, l_q);
  const int64_t i0 = (int64_t)seg * pl.seg_len + (int64_t)t * pl.chunk;
  const double q = l_q[t];
  double r = 0.0;
  double before = p0 + (q + r);
  for (int k = 0; k < pl.chunk; ++k) {
    const int64_t i = i0 + k;
    if (i >= pl.N) break;
    r += wp_weight(pl, order, w, i);
    const double here = p0 + (q + r);
    if (before <= T && T < here) {                         // exactly one element of the array
      double v;
      if (i == 0) {
        v = (double)x[0];                                  // T < acc[0]
      } else {
        const double xj = (double)x[i - 1], xi = (double)x[i];
        v = before == T ? xj : xj + (T - before) / (here - before) * (xi - xj);
      }
      out[ip] = (float)v;
    }
    before = here;
  }
}

extern "C" int mnr_weighted_percentile_partials(int64_t N) { return N > 0 ? 2 * wp_make_plan(N, 1).nseg + 1 : 0; }

extern "C" int mnr_weighted_percentile(int64_t N, const float* x_sorted, const int64_t* order, int64_t NW, const float* w,
                                       int num_p, const double* ps, double* partials, float* out, void* stream) {
  MNR_CHECK_ARG(N >= 1 && NW >= 1 && x_sorted && order && w && ps && partials && out,
                "mnr_weighted_percentile: needs N >= 1 sorted values with their order, NW >= 1 weights, the workspace and an output");
  MNR_CHECK_ARG(num_p >= 1 && num_p <= MNR_VIS_MAX_PERCENTILES, "mnr_weighted_percentile: %d percentiles, 1 to %d are taken at once",
                num_p, MNR_VIS_MAX_PERCENTILES);
  wp_ps p;
  for (int k = 0; k < MNR_VIS_MAX_PERCENTILES; ++k) {
    p.p[k] = k < num_p ? ps[k] : 0.0;
    MNR_CHECK_ARG(p.p[k] >= 0.0 && p.p[k] <= 100.0, "mnr_weighted_percentile: percentile %g is outside [0, 100]", p.p[k]);
  }
  const wp_plan pl = wp_make_plan(N, NW);
  double* seg_total = partials;
  double* P = partials + pl.nseg;
  hipLaunchKernelGGL(wp_segment_kernel, dim3(pl.nseg), dim3(WP_THREADS), 0, (hipStream_t)stream, pl, order, w, seg_total);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(wp_scan_kernel, dim3(1), dim3(WP_THREADS), 0, (hipStream_t)stream, pl.nseg, seg_total, P);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(wp_interp_kernel, dim3(pl.nseg, num_p), dim3(WP_THREADS), 0, (hipStream_t)stream, pl, x_sorted, order, w, P, p,
                     out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---------------------------------------------------------------------------
// colour map and matte

#define VIS_THREADS 256

__device__ __forceinline__ double vis_curve(int curve, double v) {
  if (curve == MNR_VIS_CURVE_LOG) return log(v + (double)MNR_F32_EPS);
  if (curve == MNR_VIS_CURVE_NEG_LOG) return -log(v + (double)MNR_F32_EPS);
  if (curve == MNR_VIS_CURVE_LN) return log(v);
  return v;
}

// jnp.mod: the result takes the sign of the divisor
__device__ __forceinline__ double vis_mod(double a, double m) {
  double r = fmod(a, m);
  if (r != 0.0 && ((r < 0.0) != (m < 0.0))) r += m;
  return r;
}

// vis.py:41-44
__device__ __forceinline__ double vis_checker(int y, int x, int width, double dark, double light) {
  const int by = (y % (2 * width)) / width, bx = (x % (2 * width)) / width;
  return (by ^ bx) ? light : dark;
}

__device__ __forceinline__ double vis_clip01(double v) {     // nan_to_num(clip(v, 0, 1))
  return v != v ? 0.0 : fmin(fmax(v, 0.0), 1.0);
}

__global__ __launch_bounds__(VIS_THREADS) void vis_cmap_kernel(mnr_vis_cmap_args a) {
  const int64_t i = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (i >= (int64_t)a.H * a.W) return;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  double lo = 0.0, hi = 1.0;
  if (a.modulus <= 0.0) {
    lo = vis_curve(a.curve, (double)a.lohi[0]);
    hi = vis_curve(a.curve, (double)a.lohi[1]);
  }
  double v[3];
  for (int c = 0; c < a.C; ++c) {
    const double cv = vis_curve(a.curve, (double)a.value[i * a.C + c]);
    if (a.modulus > 0.0) {
      v[c] = vis_mod(cv, a.modulus) / a.modulus;           // vis.py:90
    } else {
      v[c] = vis_clip01((cv - fmin(lo, hi)) / fabs(hi - lo));    // :93-94
    }
  }
  double col[3];
  if (a.lut) {
    // matplotlib's rule for a float in [0, 1]: trunc(v n), and v = 1 goes to the last entry (NaN to entry 0)
    double f = v[0] * (double)a.n_lut;
    int k = f != f ? 0 : (f >= (double)a.n_lut ? a.n_lut - 1 : (f < 0.0 ? 0 : (int)f));
    for (int c = 0; c < 3; ++c) col[c] = (double)a.lut[k * 3 + c];
  } else {
    for (int c = 0; c < 3; ++c) col[c] = v[c];
  }
  if (a.acc) {
    const double ac = (double)a.acc[i];
    const double bg = vis_checker(y, x, a.width, (double)a.dark, (double)a.light) * (1.0 - ac);
    for (int c = 0; c < 3; ++c) col[c] = col[c] * ac + bg;   // vis.py:45
  }
  for (int c = 0; c < 3; ++c) {
    if (a.out) a.out[i * 3 + c] = (float)col[c];
    if (a.out_u8) a.out_u8[i * 3 + c] = (unsigned char)(vis_clip01(col[c]) * 255.0);     // render.py:93
  }
}

extern "C" int mnr_vis_cmap(const mnr_vis_cmap_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->value && (a->out || a->out_u8), "mnr_vis_cmap: needs a value image and an output");
  MNR_CHECK_ARG(a->H > 0 && a->W > 0 && (int64_t)a->H * a->W * 3 < (1ll << 31), "mnr_vis_cmap: bad image shape [%d, %d]", a->H, a->W);
  MNR_CHECK_ARG(a->lut ? (a->C == 1 && a->n_lut >= 1) : a->C == 3,
                "mnr_vis_cmap: a colour map takes a 1-channel value, no colour map a 3-channel value (C = %d)", a->C);
  MNR_CHECK_ARG(a->curve >= MNR_VIS_CURVE_IDENTITY && a->curve <= MNR_VIS_CURVE_LN, "mnr_vis_cmap: unknown curve %d", a->curve);
  MNR_CHECK_ARG(a->modulus > 0.0 || a->lohi, "mnr_vis_cmap: needs lo / hi (a device pair) when no modulus is given");
  MNR_CHECK_ARG(!a->acc || a->width >= 1, "mnr_vis_cmap: checker width %d must be positive", a->width);
  hipLaunchKernelGGL(vis_cmap_kernel, dim3(mnr_cdiv((int64_t)a->H * a->W, VIS_THREADS)), dim3(VIS_THREADS), 0, (hipStream_t)stream, *a);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_matte_kernel(mnr_vis_matte_args a) {
  const int64_t i = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (i >= (int64_t)a.H * a.W) return;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const double ac = (double)a.acc[i];
  const double bg = vis_checker(y, x, a.width, (double)a.dark, (double)a.light) * (1.0 - ac);
  for (int c = 0; c < a.C; ++c) {
    double v;
    if (a.preop == MNR_VIS_PRE_COORD_MOD) {                // vis.py:185, :111
      double coord = (double)a.origins[i * 3 + c];         // (no directions: origins are the coordinates themselves)
      if (a.directions) coord = coord + (double)a.directions[i * 3 + c] * (double)a.distance[i];
      v = vis_mod(coord + 1.0, 2.0) / 2.0;
    } else {
      v = (double)a.x[i * a.C + c];
      if (a.preop == MNR_VIS_PRE_HALF) v = v / 2.0 + 0.5;  // :255
      if (a.preop == MNR_VIS_PRE_TANH) v = tanh(v);        // :258
    }
    a.out[i * a.C + c] = (float)(v * ac + bg);
  }
}

extern "C" int mnr_vis_matte(const mnr_vis_matte_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->acc && a->out, "mnr_vis_matte: needs acc and an output");
  MNR_CHECK_ARG(a->H > 0 && a->W > 0 && a->C >= 1 && a->C <= 4 && (int64_t)a->H * a->W * a->C < (1ll << 31),
                "mnr_vis_matte: bad image shape [%d, %d, %d]", a->H, a->W, a->C);
  MNR_CHECK_ARG(a->preop >= MNR_VIS_PRE_NONE && a->preop <= MNR_VIS_PRE_COORD_MOD, "mnr_vis_matte: unknown pre-op %d", a->preop);
  if (a->preop == MNR_VIS_PRE_COORD_MOD) {
    MNR_CHECK_ARG(a->C == 3 && a->origins && (!a->directions == !a->distance),
                  "mnr_vis_matte: the coordinate pre-op needs origins [H,W,3], and directions [H,W,3] with distance [H,W] or neither");
  } else {
    MNR_CHECK_ARG(a->x, "mnr_vis_matte: needs an image");
  }
  MNR_CHECK_ARG(a->width >= 1, "mnr_vis_matte: checker width %d must be positive", a->width);
  hipLaunchKernelGGL(vis_matte_kernel, dim3(mnr_cdiv((int64_t)a->H * a->W, VIS_THREADS)), dim3(VIS_THREADS), 0, (hipStream_t)stream, *a);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
