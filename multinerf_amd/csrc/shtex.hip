// View-dependent texture on device (gfx950): a per-texel spherical-harmonic fit over fixed world directions and the shading pass that
// evaluates it at each pixel's view direction.  include/mnerf.h states the contract (basis, weight, every operation of the fit in its
// order, the fallbacks, the lookup); tests/shtex_ref.py restates it in NumPy.  Three kernels, no atomics, no reduction across threads:
//   weights  a thread a (texel, direction) pair: one float.  The host reads it to query colours only where a direction counts.
//   fit      a thread a texel, templated on the degree so that the normal matrix's upper triangle (K (K + 1) / 2 doubles: 45 at
//            degree 2), the right-hand sides (3 K: 27) and the fallback's sums (4) are registers with constant indices: 76 doubles,
//            188 VGPRs as compiled, of the 256 a wave of a 128-thread workgroup may take (2 waves a SIMD; degree 1: 80, degree 0: 40);
//            nothing is indexed by a run-time value, so nothing goes to scratch.  Y [D,K] float64 is staged in LDS once a
//            workgroup; every lane reads the same entry (a broadcast).  A texel's D 12 B of colours are read once, and only
//            where the weight is positive; times and rates are in profiles/texture_sh.md.
//   shade    a thread a pixel: the rasteriser's texture lookup (the same formulas) on 3 K planes, then the dot with the basis.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define ST_THREADS 256
#define ST_FIT_THREADS 128

// the weight of direction d for a texel of unit normal n (include/mnerf.h): min(max(-d.n, 0), 1), NaN and -0 give +0
__host__ __device__ __forceinline__ float shtex_weight(const float* d, const float* n) {
  const float a = -mesh_dot(d, n);
  return a > 0.f ? (a < 1.f ? a : 1.f) : 0.f;
}

// the float32 basis of include/mnerf.h at a unit direction; Y has (L + 1)^2 entries
template <int L>
__host__ __device__ __forceinline__ void shtex_basis(const float* d, float* Y) {
  const float x = d[0], y = d[1], z = d[2];
  Y[0] = (float)MNR_SH_C0;
  if (L >= 1) {
    Y[1] = (float)MNR_SH_C1 * y;
    Y[2] = (float)MNR_SH_C1 * z;
    Y[3] = (float)MNR_SH_C1 * x;
  }
  if (L >= 2) {
    Y[4] = (float)MNR_SH_C2A * (x * y);
    Y[5] = (float)MNR_SH_C2A * (y * z);
    Y[6] = (float)MNR_SH_C2B * (3.f * (z * z) - 1.f);
    Y[7] = (float)MNR_SH_C2A * (x * z);
    Y[8] = (float)MNR_SH_C2C * (x * x - y * y);
  }
}

__global__ __launch_bounds__(ST_THREADS) void shtex_weights_kernel(const float* __restrict__ dirs, int64_t D, const float* __restrict__ normals,
                                                                   int64_t pairs, float* __restrict__ w) {
  const int64_t t = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= pairs) return;
  const int64_t s = t / D, k = t % D;
  const float d[3] = {dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]};
  const float n[3] = {normals[3 * s], normals[3 * s + 1], normals[3 * s + 2]};
  w[t] = shtex_weight(d, n);
}

// entry (i, j), i <= j, of the upper triangle of a K x K matrix stored row by row
#define ST_TRI(i, j) ((i) * K - (i) * ((i) - 1) / 2 + ((j) - (i)))

template <int L>
__global__ __launch_bounds__(ST_FIT_THREADS) void shtex_fit_kernel(const float* __restrict__ dirs, const double* __restrict__ Y, int D,
                                                                   const float* __restrict__ normals, const float* __restrict__ rgb, int64_t n,
                                                                   double lam, float* __restrict__ coef) {
  constexpr int K = (L + 1) * (L + 1);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* l_Y = (double*)smem;                              // [D][K]
  for (int i = threadIdx.x; i < D * K; i += ST_FIT_THREADS) l_Y[i] = Y[i];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * ST_FIT_THREADS + threadIdx.x;
  if (t >= n) return;
  const float nrm[3] = {normals[3 * t], normals[3 * t + 1], normals[3 * t + 2]};
  double M[K * (K + 1) / 2], b[K][3], s[3] = {0., 0., 0.}, sw = 0.;
#pragma unroll
  for (int i = 0; i < K * (K + 1) / 2; ++i) M[i] = 0.;
#pragma unroll
  for (int i = 0; i < K; ++i) b[i][0] = 0., b[i][1] = 0., b[i][2] = 0.;
  bool any = false;
  const float* mine = rgb + 3 * (int64_t)D * t;
  for (int k = 0; k < D; ++k) {
    const float d[3] = {dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]};
    const float wf = shtex_weight(d, nrm);
    if (!(wf > 0.f)) continue;                              // its rgb is not read
    const float c0 = mine[3 * k], c1 = mine[3 * k + 1], c2 = mine[3 * k + 2];
    if (!(mesh_finite(c0) && mesh_finite(c1) && mesh_finite(c2))) continue;
    any = true;
    const double w = (double)wf, c[3] = {(double)c0, (double)c1, (double)c2};
    const double* y = l_Y + k * K;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double tw = w * y[i];
#pragma unroll
      for (int j = i; j < K; ++j) M[ST_TRI(i, j)] += tw * y[j];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[i][ch] += tw * c[ch];
    }
    sw += w;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s[ch] += w * c[ch];
  }
  float out[K][3];
#pragma unroll
  for (int i = 0; i < K; ++i) out[i][0] = 0.f, out[i][1] = 0.f, out[i][2] = 0.f;
  if (any) {
    double tr = M[ST_TRI(0, 0)];
#pragma unroll
    for (int i = 1; i < K; ++i) tr = tr + M[ST_TRI(i, i)];
    const double mu = (lam * tr) / (double)K;
#pragma unroll
    for (int i = 1; i < K; ++i) M[ST_TRI(i, i)] += mu;
    // Cholesky in place: G_ij (j <= i) takes the place of M_ji
    bool ok = true;
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double v = M[ST_TRI(j, i)];
#pragma unroll
        for (int p = 0; p < j; ++p) v -= M[ST_TRI(p, i)] * M[ST_TRI(p, j)];
        if (j < i) {
          M[ST_TRI(j, i)] = v / M[ST_TRI(j, j)];
        } else {
          ok = ok && v > 0. && mesh_finite(v);
          M[ST_TRI(i, i)] = sqrt(v);
        }
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      double x[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        double v = b[i][ch];
#pragma unroll
        for (int p = 0; p < i; ++p) v -= M[ST_TRI(p, i)] * x[p];
        x[i] = v / M[ST_TRI(i, i)];
      }
#pragma unroll
      for (int i = K - 1; i >= 0; --i) {
        double v = x[i];
#pragma unroll
        for (int p = i + 1; p < K; ++p) v -= M[ST_TRI(i, p)] * x[p];
        x[i] = v / M[ST_TRI(i, i)];
      }
#pragma unroll
      for (int i = 0; i < K; ++i) {
        out[i][ch] = (float)x[i];
        ok = ok && mesh_finite(out[i][ch]);
      }
    }
    if (!ok) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float mean = (float)((s[ch] / sw) / l_Y[0]);
        out[0][ch] = mesh_finite(mean) ? mean : 0.f;
#pragma unroll
        for (int i = 1; i < K; ++i) out[i][ch] = 0.f;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) coef[3 * ((int64_t)K * t + i) + ch] = out[i][ch];
  }
}

template <int L>
__device__ __forceinline__ void shtex_shade_pixel(const mnr_shtex_shade_args& a, int64_t t, float* __restrict__ rgb) {
  constexpr int K = (L + 1) * (L + 1);
  const int64_t f = a.face[t];
  int id[3];
  if (f < 0 || f >= a.n_faces || !mesh_face_ids(a.faces, f, a.n_verts, id)) return;
  const float l[3] = {a.bary[3 * t], a.bary[3 * t + 1], a.bary[3 * t + 2]};
  float X[3], d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    X[c] = (l[0] * a.verts[3 * (int64_t)id[0] + c] + l[1] * a.verts[3 * (int64_t)id[1] + c]) + l[2] * a.verts[3 * (int64_t)id[2] + c];
  }
  mesh_sub(X, a.origin, d);
  if (!mesh_normalise(d)) d[0] = 0.f, d[1] = 0.f, d[2] = 1.f;
  float Y[K];
  shtex_basis<L>(d, Y);
  // the texture lookup of raster_shade_kernel (include/mnerf.h, the rasteriser's section)
  const float* uv = a.uv + 6 * f;
  const float u = (l[0] * uv[0] + l[1] * uv[2]) + l[2] * uv[4], v = (l[0] * uv[1] + l[1] * uv[3]) + l[2] * uv[5];
  const float x = u * (float)a.Wt - 0.5f, y = (1.f - v) * (float)a.Ht - 0.5f;
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  const int xi = (int)fminf(fmaxf(xf, -1.f), (float)a.Wt), yi = (int)fminf(fmaxf(yf, -1.f), (float)a.Ht);   // fmaxf(NaN, -1) = -1
  const int xa = min(max(xi, 0), a.Wt - 1), xb = min(max(xi + 1, 0), a.Wt - 1);
  const int ya = min(max(yi, 0), a.Ht - 1), yb = min(max(yi + 1, 0), a.Ht - 1);
  const float* taa = a.sh + 3 * K * ((int64_t)ya * a.Wt + xa);
  const float* tab = a.sh + 3 * K * ((int64_t)ya * a.Wt + xb);
  const float* tba = a.sh + 3 * K * ((int64_t)yb * a.Wt + xa);
  const float* tbb = a.sh + 3 * K * ((int64_t)yb * a.Wt + xb);
  float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = (1.f - fx) * taa[3 * j + c] + fx * tab[3 * j + c];
      const float bot = (1.f - fx) * tba[3 * j + c] + fx * tbb[3 * j + c];
      const float val = (1.f - fy) * top + fy * bot;
      r[c] = j == 0 ? Y[0] * val : r[c] + Y[j] * val;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[3 * t + c] = r[c] > 0.f ? (r[c] < 1.f ? r[c] : 1.f) : 0.f;   // NaN: 0
}

__global__ __launch_bounds__(ST_THREADS) void shtex_shade_kernel(mnr_shtex_shade_args a, float* __restrict__ rgb) {
  const int64_t t = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= (int64_t)a.H * a.W) return;
  if (a.degree == 0) shtex_shade_pixel<0>(a, t, rgb);
  else if (a.degree == 1) shtex_shade_pixel<1>(a, t, rgb);
  else shtex_shade_pixel<2>(a, t, rgb);
}

static int st_check_dirs(const char* name, int64_t D, int64_t n) {
  MNR_CHECK_ARG(D >= 1 && D <= MNR_SHTEX_MAX_DIRS, "%s: %lld directions: must lie in 1 .. %d", name, (long long)D, MNR_SHTEX_MAX_DIRS);
  MNR_CHECK_ARG(n >= 0 && n < (1ll << 31), "%s: %lld texels: must lie in 0 .. 2^31 - 1", name, (long long)n);   // (n D < 2^40)
  return MNR_OK;
}

extern "C" int mnr_shtex_weights(const float* dirs, int64_t n_dirs, const float* normals, int64_t n, float* w, void* stream) {
  const int st = st_check_dirs("mnr_shtex_weights", n_dirs, n);
  if (st != MNR_OK) return st;
  const int64_t pairs = n * n_dirs;
  MNR_CHECK_ARG(pairs <= ((1ll << 31) - 1) * ST_THREADS, "mnr_shtex_weights: %lld pairs are more than one launch takes", (long long)pairs);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(dirs && normals && w, "mnr_shtex_weights: needs dirs [D,3], normals [n,3] and w [n,D]");
  hipLaunchKernelGGL(shtex_weights_kernel, dim3((unsigned)mnr_cdiv(pairs, ST_THREADS)), dim3(ST_THREADS), 0, (hipStream_t)stream, dirs, n_dirs, normals,
                     pairs, w);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_shtex_fit(const float* dirs, const double* Y, int64_t n_dirs, int degree, const float* normals, const float* rgb, int64_t n,
                             double lam, float* coef, void* stream) {
  const int st = st_check_dirs("mnr_shtex_fit", n_dirs, n);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(degree >= 0 && degree <= MNR_SHTEX_MAX_DEGREE, "mnr_shtex_fit: degree = %d must lie in 0 .. %d", degree, MNR_SHTEX_MAX_DEGREE);
  MNR_CHECK_ARG(lam >= 0. && lam <= 1.7976931348623157e308, "mnr_shtex_fit: lam = %g must be finite and not negative", lam);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(dirs && Y && normals && rgb && coef, "mnr_shtex_fit: needs dirs [D,3], Y [D,K], normals [n,3], rgb [n,D,3] and coef [n,K,3]");
  const int K = (degree + 1) * (degree + 1), D = (int)n_dirs;
  const dim3 grid((unsigned)mnr_cdiv(n, ST_FIT_THREADS)), block(ST_FIT_THREADS);
  const size_t lds = sizeof(double) * (size_t)D * K;       // at most 512 x 9 x 8 B = 36 KiB
  if (degree == 0) hipLaunchKernelGGL(shtex_fit_kernel<0>, grid, block, lds, (hipStream_t)stream, dirs, Y, D, normals, rgb, n, lam, coef);
  else if (degree == 1) hipLaunchKernelGGL(shtex_fit_kernel<1>, grid, block, lds, (hipStream_t)stream, dirs, Y, D, normals, rgb, n, lam, coef);
  else hipLaunchKernelGGL(shtex_fit_kernel<2>, grid, block, lds, (hipStream_t)stream, dirs, Y, D, normals, rgb, n, lam, coef);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_shtex_shade(const mnr_shtex_shade_args* a, float* rgb, void* stream) {
  MNR_CHECK_ARG(a, "mnr_shtex_shade: needs its arguments");
  const int st = md_check_mesh("mnr_shtex_shade", a->verts, a->n_verts, a->faces, a->n_faces);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(a->H >= 1 && a->W >= 1, "mnr_shtex_shade: an image of %d x %d pixels: both sides must be at least 1", a->H, a->W);
  MNR_CHECK_ARG(a->degree >= 0 && a->degree <= MNR_SHTEX_MAX_DEGREE, "mnr_shtex_shade: degree = %d must lie in 0 .. %d", a->degree,
                MNR_SHTEX_MAX_DEGREE);
  MNR_CHECK_ARG(a->Ht >= 1 && a->Wt >= 1 && a->Ht <= (1 << 24) && a->Wt <= (1 << 24), "mnr_shtex_shade: 1 .. 2^24 texels a side, has %d x %d", a->Ht,
                a->Wt);
  MNR_CHECK_ARG(mesh_finite(a->origin[0]) && mesh_finite(a->origin[1]) && mesh_finite(a->origin[2]), "mnr_shtex_shade: the origin must be finite");
  MNR_CHECK_ARG(a->face && a->bary && a->sh && rgb && (a->n_faces == 0 || a->uv),
                "mnr_shtex_shade: needs face [H,W], bary [H,W,3], uv [n_faces,3,2], sh [Ht,Wt,K,3] and rgb [H,W,3]");
  const int64_t pixels = (int64_t)a->H * a->W;
  hipLaunchKernelGGL(shtex_shade_kernel, dim3((unsigned)mnr_cdiv(pixels, ST_THREADS)), dim3(ST_THREADS), 0, (hipStream_t)stream, *a, rgb);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
