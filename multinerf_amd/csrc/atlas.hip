// Texture atlas on device (gfx950): per-face charts in a regular grid of cells.  include/mnerf.h states the contract (layout,
// ownership, texel -> surface, surface -> UV, the footprint Gaussian, every float32 operation in its order); tests/atlas_ref.py
// restates it in NumPy.  Three kernels, all one thread per element, no shared memory and no read-modify-write of global memory:
//   samples  a thread a sample s = cell c (c + 1) + Y (c + 1) + X.  The 64 consecutive samples of a wave lie in at most
//            ceil(64 / (c (c + 1))) + 1 cells, so the face's 3 indices and 18 floats are the same addresses across most of a wave
//            (one cache line each, broadcast) and the 19 outputs a sample are stored contiguously per array: the kernel is bound
//            by its 76 B of stores a sample.
//   store    a thread a sample: the quantised colour goes to the texel the sample came from (3 bytes + 1 mask byte; consecutive
//            samples of a cell row are consecutive texels).  Each texel belongs to one sample.
//   uvs      a thread a face, 6 floats.
// The sample kernel and the UV kernel are inverses of each other: both take a face's anchor texel and step from atlas_chart_of.
// Every index read from faces is checked against [0, n_verts) before it is used as one.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define AT_THREADS 256

static_assert(MNR_ATLAS_MIN_CELL == 3, "b = x' / (c - 2) needs c - 2 >= 1");

// A face's chart: the absolute texel of its v0 (x' = y' = 0) and the step of one face-local texel along both atlas axes.
struct atlas_chart {
  int64_t x0, y0;
  int step;
};

__host__ __device__ __forceinline__ atlas_chart atlas_chart_of(int64_t face, int c, int cols) {
  const int64_t cell = face >> 1;
  const int64_t X0 = (cell % cols) * (int64_t)(c + 1), Y0 = (cell / cols) * (int64_t)c;
  atlas_chart ch;
  const bool upper = (face & 1) != 0;
  ch.x0 = upper ? X0 + c : X0;
  ch.y0 = upper ? Y0 + c - 1 : Y0;
  ch.step = upper ? -1 : 1;
  return ch;
}

// Sample s of the atlas: its absolute texel, the face that owns it and its face-local texel.
struct atlas_texel {
  int64_t X, Y, face;
  int xl, yl;
};

__host__ __device__ __forceinline__ atlas_texel atlas_texel_of(int64_t s, int c, int cols) {
  const int64_t per_cell = (int64_t)c * (c + 1);
  const int64_t cell = s / per_cell;
  const int r = (int)(s % per_cell);
  const int Y = r / (c + 1), X = r % (c + 1);
  atlas_texel t;
  t.face = 2 * cell + ((X + Y <= c - 1) ? 0 : 1);
  t.X = (cell % cols) * (int64_t)(c + 1) + X;
  t.Y = (cell / cols) * (int64_t)c + Y;
  const atlas_chart ch = atlas_chart_of(t.face, c, cols);
  t.xl = (int)(t.X - ch.x0) * ch.step;
  t.yl = (int)(t.Y - ch.y0) * ch.step;
  return t;
}

__global__ __launch_bounds__(AT_THREADS) void atlas_samples_kernel(mnr_atlas_args a, int64_t s0, int64_t n, float* __restrict__ means,
                                                                   float* __restrict__ covs, float* __restrict__ normals,
                                                                   float* __restrict__ viewdirs, int* __restrict__ face) {
  const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
  if (t >= n) return;
  const atlas_texel tx = atlas_texel_of(s0 + t, a.c, a.cols);
  float p[3] = {0.f, 0.f, 0.f}, cov[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 1.f}, vd[3] = {0.f, 0.f, 1.f};
  int owner = -1;
  bool valid = tx.face < a.n_faces;
  int id[3] = {0, 0, 0};
  if (valid) {                                              // (written out: mesh_face_ids and mesh_cross give this kernel other device code)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      id[k] = a.faces[3 * tx.face + k];
      valid = valid && id[k] >= 0 && id[k] < a.n_verts;
    }
  }
  if (valid) {
    float v[3][3], vn[3][3];
    float check = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        v[k][d] = a.verts[3 * (int64_t)id[k] + d];
        vn[k][d] = a.normals[3 * (int64_t)id[k] + d];
        valid = valid && mesh_finite(v[k][d]);
      }
    }
    const float den = (float)(a.c - 2);
    const float b1 = (float)tx.xl / den, b2 = (float)tx.yl / den;
    const float b0 = (1.f - b1) - b2;
    float ea[3], eb[3], e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      p[d] = (b0 * v[0][d] + b1 * v[1][d]) + b2 * v[2][d];
      e1[d] = v[1][d] - v[0][d];
      e2[d] = v[2][d] - v[0][d];
      ea[d] = e1[d] / den;
      eb[d] = e2[d] / den;
      check += p[d] - p[d];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        cov[3 * i + j] = a.cov_scale * (ea[i] * ea[j] + eb[i] * eb[j]);
        check += cov[3 * i + j] - cov[3 * i + j];
      }
    }
    valid = valid && check == 0.f;                          // a mean or a covariance entry that is not finite
    if (valid) {
      owner = (int)tx.face;
      float nn[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) nn[d] = (b0 * vn[0][d] + b1 * vn[1][d]) + b2 * vn[2][d];
      bool unit = mesh_normalise(nn);
      if (!unit) {
        nn[0] = e1[1] * e2[2] - e1[2] * e2[1];
        nn[1] = e1[2] * e2[0] - e1[0] * e2[2];
        nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
        unit = mesh_normalise(nn);
      }
      if (unit) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          nrm[d] = nn[d];
          vd[d] = -nn[d];
        }
      }
    } else {
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = 0.f;
#pragma unroll
      for (int d = 0; d < 9; ++d) cov[d] = 0.f;
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    means[3 * t + d] = p[d];
    normals[3 * t + d] = nrm[d];
    viewdirs[3 * t + d] = vd[d];
  }
#pragma unroll
  for (int d = 0; d < 9; ++d) covs[9 * t + d] = cov[d];
  face[t] = owner;
}

__global__ __launch_bounds__(AT_THREADS) void atlas_store_kernel(mnr_atlas_args a, int64_t s0, int64_t n, const float* __restrict__ rgb,
                                                                 const int* __restrict__ face, unsigned char* __restrict__ atlas,
                                                                 unsigned char* __restrict__ mask, float* __restrict__ atlas_f32) {
  const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
  if (t >= n) return;
  if (face[t] < 0) return;
  const atlas_texel tx = atlas_texel_of(s0 + t, a.c, a.cols);
  if (tx.X >= a.W || tx.Y >= a.H) return;                   // cannot happen for s below the total the entry checked
  const int64_t at = tx.Y * (int64_t)a.W + tx.X;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float x = rgb[3 * t + d];
    const float q = fminf(fmaxf(x, 0.f), 1.f);              // fmaxf(NaN, 0) = 0
    atlas[3 * at + d] = (unsigned char)(int)floorf(q * 255.f + 0.5f);
    if (atlas_f32 != nullptr) atlas_f32[3 * at + d] = x;
  }
  mask[at] = 255;
}

__global__ __launch_bounds__(AT_THREADS) void atlas_uvs_kernel(int64_t T, int c, int cols, int W, int H, float* __restrict__ uv) {
  const int64_t f = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
  if (f >= T) return;
  const atlas_chart ch = atlas_chart_of(f, c, cols);
  const int64_t reach = (int64_t)ch.step * (c - 2);
  const float fw = (float)W, fh = (float)H;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float px = (float)(ch.x0 + (k == 1 ? reach : 0)) + 0.5f;
    const float py = (float)(ch.y0 + (k == 2 ? reach : 0)) + 0.5f;
    uv[6 * f + 2 * k] = px / fw;
    uv[6 * f + 2 * k + 1] = 1.f - py / fh;
  }
}

// c, cols, W, H and the counts against the contract; *total = the number of samples.
static int at_check(const char* name, const mnr_atlas_args* a, int64_t* total) {
  MNR_CHECK_ARG(a, "%s: needs its arguments", name);
  MNR_CHECK_ARG(a->n_verts >= 0 && a->n_verts < (1ll << 31) && a->n_faces >= 0 && a->n_faces < (1ll << 31),
                "%s: %lld vertices and %lld faces, both must lie in 0 .. 2^31 - 1", name, (long long)a->n_verts, (long long)a->n_faces);
  MNR_CHECK_ARG(a->c >= MNR_ATLAS_MIN_CELL, "%s: the cell size c = %d must be at least %d", name, a->c, MNR_ATLAS_MIN_CELL);
  MNR_CHECK_ARG(a->cols >= 1, "%s: cols = %d must be at least 1", name, a->cols);
  const int64_t ncells = (a->n_faces + 1) / 2;
  const int64_t rows = (ncells + a->cols - 1) / a->cols;
  const int64_t W = ncells == 0 ? 0 : (int64_t)a->cols * ((int64_t)a->c + 1), H = rows * (int64_t)a->c;
  MNR_CHECK_ARG(W < (1ll << 31) && H < (1ll << 31), "%s: an atlas of %lld x %lld texels: both sides must stay below 2^31", name, (long long)W,
                (long long)H);
  MNR_CHECK_ARG(a->W == W && a->H == H, "%s: W x H = %d x %d, the contract gives %lld x %lld for %lld faces, c = %d, cols = %d", name, a->W, a->H,
                (long long)W, (long long)H, (long long)a->n_faces, a->c, a->cols);
  *total = ncells * (int64_t)a->c * ((int64_t)a->c + 1);   // <= W H < 2^62
  return MNR_OK;
}

static int at_check_chunk(const char* name, int64_t s0, int64_t n, int64_t total) {
  MNR_CHECK_ARG(s0 >= 0 && n >= 0 && n < (1ll << 31) && s0 <= total && n <= total - s0,
                "%s: samples %lld .. %lld + %lld of %lld: a chunk lies inside the atlas and has fewer than 2^31 samples", name, (long long)s0,
                (long long)s0, (long long)n, (long long)total);
  return MNR_OK;
}

extern "C" int mnr_atlas_samples(const mnr_atlas_args* a, int64_t s0, int64_t n, float* means, float* covs, float* normals, float* viewdirs,
                                 int* face, void* stream) {
  int64_t total = 0;
  int st = at_check("mnr_atlas_samples", a, &total);
  if (st != MNR_OK) return st;
  st = at_check_chunk("mnr_atlas_samples", s0, n, total);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(a->cov_scale >= 0.f && a->cov_scale <= MNR_F32_MAX, "mnr_atlas_samples: cov_scale = %g must be finite and not negative",
                (double)a->cov_scale);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(a->faces && (a->n_verts == 0 || (a->verts && a->normals)), "mnr_atlas_samples: needs verts, normals [n_verts,3] and faces [n_faces,3]");
  MNR_CHECK_ARG(means && covs && normals && viewdirs && face,
                "mnr_atlas_samples: needs means [n,3], covs [n,3,3], normals [n,3], viewdirs [n,3] and face [n]");
  hipLaunchKernelGGL(atlas_samples_kernel, dim3((unsigned)mnr_cdiv(n, AT_THREADS)), dim3(AT_THREADS), 0, (hipStream_t)stream, *a, s0, n, means,
                     covs, normals, viewdirs, face);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_atlas_store(const mnr_atlas_args* a, int64_t s0, int64_t n, const float* rgb, const int* face, unsigned char* atlas,
                               unsigned char* mask, float* atlas_f32, void* stream) {
  int64_t total = 0;
  int st = at_check("mnr_atlas_store", a, &total);
  if (st != MNR_OK) return st;
  st = at_check_chunk("mnr_atlas_store", s0, n, total);
  if (st != MNR_OK) return st;
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(rgb && face && atlas && mask, "mnr_atlas_store: needs rgb [n,3], face [n], atlas [H,W,3] and mask [H,W]");
  hipLaunchKernelGGL(atlas_store_kernel, dim3((unsigned)mnr_cdiv(n, AT_THREADS)), dim3(AT_THREADS), 0, (hipStream_t)stream, *a, s0, n, rgb, face,
                     atlas, mask, atlas_f32);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_atlas_uvs(const mnr_atlas_args* a, float* uv, void* stream) {
  int64_t total = 0;
  const int st = at_check("mnr_atlas_uvs", a, &total);
  if (st != MNR_OK) return st;
  if (a->n_faces == 0) return MNR_OK;
  MNR_CHECK_ARG(uv, "mnr_atlas_uvs: needs uv [n_faces,3,2]");
  hipLaunchKernelGGL(atlas_uvs_kernel, dim3((unsigned)mnr_cdiv(a->n_faces, AT_THREADS)), dim3(AT_THREADS), 0, (hipStream_t)stream, a->n_faces,
                     a->c, a->cols, a->W, a->H, uv);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
