// Mesh rasteriser on device (gfx950): a visibility buffer by 2D homogeneous rasterisation (Olano and Greer 1997) and a shading pass.
// include/mnerf.h states the contract (every float32 operation in its order, coverage, tie rule, key, shading); tests/raster_ref.py
// restates it in NumPy, every face against every pixel.  Nothing is clipped: the edge functions come from the homogeneous
// vertices, so a triangle that crosses the camera plane is no special case.
//   fill        vis = all ones, the large-face counter = 0
//   small       a thread a face: setup, bounding box, and, when the box has at most `threshold` pixels, a walk over it.  The faces
//               with a larger box are compacted into a list (one atomicAdd a wave: __ballot / __popcll of the flagged lanes).
//   large       a workgroup a listed face, striding over the box: the setup's 3 indices and 9 floats are one address across
//               the workgroup (broadcast), consecutive threads test consecutive pixels of a box row.
//   shade       a thread a pixel: decode the winner, recompute its edge functions with the SAME rs_setup / rs_cover, interpolate.
// The resolve is atomicMin on a 64-bit key (depth bits << 32 | face): an integer minimum does not depend on the order of arrival,
// so two runs agree bit for bit; there is no floating-point atomic.  The list's ORDER does depend on arrival, its content and the
// minimum do not.  Every index read from faces, the list and the buffer is checked before it is used as one.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define RS_THREADS 256
#define RS_EMPTY 0xffffffffffffffffull

// A face's edge functions, already multiplied by s = sign(det): E_i(px, py) = (n[i][0] px + n[i][1] py) + n[i][2].
struct rs_face {
  float n[3][3];
  float h[3][3];                                            // homogeneous vertices (u zc, v zc, zc)
  float adet;                                               // |det|
  float s;                                                  // +1 or -1
};

__host__ __device__ __forceinline__ bool rs_tie(const float* a) { return a[0] > 0.f || (a[0] == 0.f && (a[1] > 0.f || (a[1] == 0.f && a[2] > 0.f))); }

// false: the face is skipped (an index outside the vertices, a homogeneous coordinate that is not finite, det 0 or not finite)
__host__ __device__ __forceinline__ bool rs_setup(const mnr_raster_args& a, int64_t f, rs_face& o) {
  int id[3];
  if (!mesh_face_ids(a.faces, f, a.n_verts, id)) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = a.verts[3 * (int64_t)id[k]], y = a.verts[3 * (int64_t)id[k] + 1], z = a.verts[3 * (int64_t)id[k] + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      o.h[k][r] = ((a.proj[4 * r] * x + a.proj[4 * r + 1] * y) + a.proj[4 * r + 2] * z) + a.proj[4 * r + 3];
      ok = ok && mesh_finite(o.h[k][r]);
    }
  }
  if (!ok) return false;
  float n[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) mesh_cross(o.h[(i + 1) % 3], o.h[(i + 2) % 3], n[i]);
  const float det = mesh_dot(n[0], o.h[0]);
  if (!mesh_finite(det) || det == 0.f) return false;
  o.s = det > 0.f ? 1.f : -1.f;
  o.adet = fabsf(det);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int d = 0; d < 3; ++d) o.n[i][d] = o.s * n[i][d];
  }
  return true;
}

// the coverage test of a pixel (x, y) of the face's box; E, S and zc are written whatever it returns
__host__ __device__ __forceinline__ bool rs_cover(const rs_face& fc, int x, int y, float near, float* E, float* S, float* zc) {
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  bool in = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    E[i] = (fc.n[i][0] * px + fc.n[i][1] * py) + fc.n[i][2];
    in = in && (E[i] > 0.f || (E[i] == 0.f && rs_tie(fc.n[i])));
  }
  *S = (E[0] + E[1]) + E[2];
  *zc = fc.adet / *S;
  return in && *S > 0.f && mesh_finite(*zc) && *zc > near;
}

// the face's pixel box [x0, x1] x [y0, y1], a clause of the coverage test (include/mnerf.h): both kernels visit these pixels only; false: none
__host__ __device__ __forceinline__ bool rs_box(const rs_face& fc, int W, int H, int* x0, int* x1, int* y0, int* y1) {
  *x0 = 0, *y0 = 0, *x1 = W - 1, *y1 = H - 1;
  if (fc.h[0][2] <= 0.f && fc.h[1][2] <= 0.f && fc.h[2][2] <= 0.f) return false;      // wholly behind the camera plane
  if (!(fc.h[0][2] > 0.f && fc.h[1][2] > 0.f && fc.h[2][2] > 0.f)) return true;       // across it: the whole image
  float lo[2], hi[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const float a = fc.h[0][d] / fc.h[0][2], b = fc.h[1][d] / fc.h[1][2], c = fc.h[2][d] / fc.h[2][2];   // finite or an infinity
    lo[d] = fmaxf(floorf(fminf(fminf(a, b), c)) - 1.f, 0.f);
    hi[d] = fminf(floorf(fmaxf(fmaxf(a, b), c)) + 1.f, (float)((d == 0 ? W : H) - 1));
    if (!(lo[d] <= hi[d])) return false;
  }
  *x0 = (int)lo[0], *x1 = (int)hi[0], *y0 = (int)lo[1], *y1 = (int)hi[1];
  return true;
}

__device__ __forceinline__ void rs_resolve(unsigned long long* vis, int W, int x, int y, float zc, int64_t f) {
  const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, zc) << 32) | (unsigned long long)(unsigned)f;
  atomicMin(&vis[(int64_t)y * W + x], key);
}

__global__ __launch_bounds__(RS_THREADS) void raster_fill_kernel(int64_t n, unsigned long long* __restrict__ vis, int* __restrict__ count) {
  const int64_t t = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (t < n) vis[t] = RS_EMPTY;
  if (t == 0) *count = 0;
}

__global__ __launch_bounds__(RS_THREADS) void raster_small_kernel(mnr_raster_args a, unsigned long long* __restrict__ vis, int* __restrict__ list,
                                                                  int* __restrict__ count) {
  const int64_t f = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  rs_face fc;
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
  bool live = f < a.n_faces && rs_setup(a, f, fc);
  live = live && !(a.cull == MNR_RASTER_CULL_BACK && fc.s > 0.f) && rs_box(fc, a.W, a.H, &x0, &x1, &y0, &y1);
  const bool large = live && (int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) > a.threshold;
  const unsigned long long bal = __ballot(large);           // every thread of the wave gets here
  if (bal != 0ull) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == __ffsll(bal) - 1) base = atomicAdd(count, __popcll(bal));
    base = __shfl(base, __ffsll(bal) - 1);
    if (large) {
      const int at = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (at >= 0 && at < a.n_faces) list[at] = (int)f;
    }
  }
  if (!live || large) return;
  float E[3], S, zc;
  for (int y = y0; y <= y1; ++y) {
    for (int x = x0; x <= x1; ++x) {
      if (rs_cover(fc, x, y, a.near, E, &S, &zc)) rs_resolve(vis, a.W, x, y, zc, f);
    }
  }
}

__global__ __launch_bounds__(RS_THREADS) void raster_large_kernel(mnr_raster_args a, unsigned long long* __restrict__ vis,
                                                                  const int* __restrict__ list, const int* __restrict__ count) {
  const int64_t n = min((int64_t)*count, a.n_faces);
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t f = list[i];
    rs_face fc;
    int x0, x1, y0, y1;
    if (f < 0 || f >= a.n_faces || !rs_setup(a, f, fc) || !rs_box(fc, a.W, a.H, &x0, &x1, &y0, &y1)) continue;   // (uniform over the workgroup)
    const int bw = x1 - x0 + 1;
    const int64_t pixels = (int64_t)bw * (y1 - y0 + 1);
    float E[3], S, zc;
    for (int64_t p = threadIdx.x; p < pixels; p += RS_THREADS) {
      const int x = x0 + (int)(p % bw), y = y0 + (int)(p / bw);
      if (rs_cover(fc, x, y, a.near, E, &S, &zc)) rs_resolve(vis, a.W, x, y, zc, f);
    }
  }
}

__device__ __forceinline__ float rs_texel(const mnr_raster_args& a, int x, int y, int d) {
  const int64_t at = 3 * ((int64_t)y * a.Wt + x) + d;
  return a.texture_u8 ? (float)((const unsigned char*)a.texture)[at] / 255.f : ((const float*)a.texture)[at];
}

__global__ __launch_bounds__(RS_THREADS) void raster_shade_kernel(mnr_raster_args a, const unsigned long long* __restrict__ vis,
                                                                  int* __restrict__ face, float* __restrict__ depth, float* __restrict__ acc,
                                                                  float* __restrict__ bary, float* __restrict__ normals, float* __restrict__ rgb) {
  const int64_t t = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (t >= (int64_t)a.H * a.W) return;
  const unsigned long long key = vis[t];
  const int64_t f = (int64_t)(key & 0xffffffffull);
  rs_face fc;
  float E[3] = {0.f, 0.f, 0.f}, S = 0.f, zc = 0.f;
  float l[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f}, col[3] = {a.bg[0], a.bg[1], a.bg[2]};
  bool hit = key != RS_EMPTY && f < a.n_faces && rs_setup(a, f, fc);
  if (hit) {
    rs_cover(fc, (int)(t % a.W), (int)(t / a.W), a.near, E, &S, &zc);
    int id[3];
    float vn[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      id[k] = a.faces[3 * f + k];                           // inside the vertices: rs_setup has checked
      l[k] = E[k] / S;
#pragma unroll
      for (int d = 0; d < 3; ++d) vn[k][d] = a.normals[3 * (int64_t)id[k] + d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) nrm[d] = (l[0] * vn[0][d] + l[1] * vn[1][d]) + l[2] * vn[2][d];
    bool unit = mesh_normalise(nrm);
    if (!unit) {
      float e1[3], e2[3];
      mesh_sub(a.verts + 3 * (int64_t)id[1], a.verts + 3 * (int64_t)id[0], e1);
      mesh_sub(a.verts + 3 * (int64_t)id[2], a.verts + 3 * (int64_t)id[0], e2);
      mesh_cross(e1, e2, nrm);
      unit = mesh_normalise(nrm);
    }
    if (!unit) nrm[0] = 0.f, nrm[1] = 0.f, nrm[2] = 1.f;
    if (a.colors != nullptr) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int64_t at = 3 * (int64_t)id[k] + d;
          c[k] = a.colors_u8 ? (float)((const unsigned char*)a.colors)[at] / 255.f : ((const float*)a.colors)[at];
        }
        col[d] = (l[0] * c[0] + l[1] * c[1]) + l[2] * c[2];
      }
    } else if (a.texture != nullptr) {
      const float* uv = a.uv + 6 * f;
      const float u = (l[0] * uv[0] + l[1] * uv[2]) + l[2] * uv[4], v = (l[0] * uv[1] + l[1] * uv[3]) + l[2] * uv[5];
      const float x = u * (float)a.Wt - 0.5f, y = (1.f - v) * (float)a.Ht - 0.5f;
      const float xf = floorf(x), yf = floorf(y);
      const float fx = x - xf, fy = y - yf;
      const int xi = (int)fminf(fmaxf(xf, -1.f), (float)a.Wt), yi = (int)fminf(fmaxf(yf, -1.f), (float)a.Ht);   // fmaxf(NaN, -1) = -1
      const int xa = min(max(xi, 0), a.Wt - 1), xb = min(max(xi + 1, 0), a.Wt - 1);
      const int ya = min(max(yi, 0), a.Ht - 1), yb = min(max(yi + 1, 0), a.Ht - 1);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float top = (1.f - fx) * rs_texel(a, xa, ya, d) + fx * rs_texel(a, xb, ya, d);
        const float bot = (1.f - fx) * rs_texel(a, xa, yb, d) + fx * rs_texel(a, xb, yb, d);
        col[d] = (1.f - fy) * top + fy * bot;
      }
    } else {
#pragma unroll
      for (int d = 0; d < 3; ++d) col[d] = 0.5f + 0.5f * nrm[d];
    }
  }
  face[t] = hit ? (int)f : -1;
  depth[t] = hit ? zc : 0.f;
  acc[t] = hit ? 1.f : 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    bary[3 * t + d] = l[d];
    normals[3 * t + d] = nrm[d];
    rgb[3 * t + d] = col[d];
  }
}

static int rs_check(const char* name, const mnr_raster_args* a) {
  MNR_CHECK_ARG(a, "%s: needs its arguments", name);
  MNR_CHECK_ARG(a->n_verts >= 0 && a->n_verts < (1ll << 31) && a->n_faces >= 0 && a->n_faces < (1ll << 31) - 1,
                "%s: %lld vertices and %lld faces: vertices must lie in 0 .. 2^31 - 1, faces in 0 .. 2^31 - 2", name, (long long)a->n_verts,
                (long long)a->n_faces);
  MNR_CHECK_ARG(a->H >= 1 && a->W >= 1, "%s: an image of %d x %d pixels: both sides must be at least 1", name, a->H, a->W);
  MNR_CHECK_ARG(a->near > 0.f && a->near <= MNR_F32_MAX, "%s: near = %g must be positive and finite", name, (double)a->near);
  MNR_CHECK_ARG(a->n_faces == 0 || (a->faces && (a->n_verts == 0 || a->verts)), "%s: needs verts [n_verts,3] and faces [n_faces,3]", name);
  return MNR_OK;
}

extern "C" int mnr_raster_visibility(const mnr_raster_args* a, uint64_t* vis, int* list, int* count, void* stream) {
  const int st = rs_check("mnr_raster_visibility", a);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(a->cull == MNR_RASTER_CULL_NONE || a->cull == MNR_RASTER_CULL_BACK, "mnr_raster_visibility: cull = %d is neither NONE nor BACK",
                a->cull);
  MNR_CHECK_ARG(a->threshold >= 0, "mnr_raster_visibility: threshold = %lld must not be negative", (long long)a->threshold);
  MNR_CHECK_ARG(vis && count && (a->n_faces == 0 || list), "mnr_raster_visibility: needs vis [H,W], list [n_faces] and count [1]");
  const int64_t pixels = (int64_t)a->H * a->W;
  hipLaunchKernelGGL(raster_fill_kernel, dim3((unsigned)mnr_cdiv(pixels, RS_THREADS)), dim3(RS_THREADS), 0, (hipStream_t)stream, pixels,
                     (unsigned long long*)vis, count);
  MNR_CHECK_LAUNCH();
  if (a->n_faces == 0) return MNR_OK;
  hipLaunchKernelGGL(raster_small_kernel, dim3((unsigned)mnr_cdiv(a->n_faces, RS_THREADS)), dim3(RS_THREADS), 0, (hipStream_t)stream, *a,
                     (unsigned long long*)vis, list, count);
  MNR_CHECK_LAUNCH();
  const int64_t wgs = a->n_faces < 8ll * mnr_cu_count() ? a->n_faces : 8ll * mnr_cu_count();
  hipLaunchKernelGGL(raster_large_kernel, dim3((unsigned)wgs), dim3(RS_THREADS), 0, (hipStream_t)stream, *a, (unsigned long long*)vis, list, count);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_raster_shade(const mnr_raster_args* a, const uint64_t* vis, int* face, float* depth, float* acc, float* bary, float* normals,
                                float* rgb, void* stream) {
  const int st = rs_check("mnr_raster_shade", a);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(a->n_faces == 0 || a->n_verts == 0 || a->normals, "mnr_raster_shade: needs normals [n_verts,3]");
  MNR_CHECK_ARG(!(a->colors && a->texture), "mnr_raster_shade: colors and texture are both given: the colour has one source");
  MNR_CHECK_ARG(!a->texture || (a->uv && a->Ht >= 1 && a->Wt >= 1 && a->Ht <= (1 << 24) && a->Wt <= (1 << 24)),
                "mnr_raster_shade: a texture needs uv [n_faces,3,2] and 1 .. 2^24 texels a side, has %d x %d", a->Ht, a->Wt);
  MNR_CHECK_ARG(vis && face && depth && acc && bary && normals && rgb,
                "mnr_raster_shade: needs vis, face, depth, acc [H,W] and bary, normals, rgb [H,W,3]");
  const int64_t pixels = (int64_t)a->H * a->W;
  hipLaunchKernelGGL(raster_shade_kernel, dim3((unsigned)mnr_cdiv(pixels, RS_THREADS)), dim3(RS_THREADS), 0, (hipStream_t)stream, *a,
                     (const unsigned long long*)vis, face, depth, acc, bary, normals, rgb);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
