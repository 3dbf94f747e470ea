// Mesh geometry on device (gfx950): the squared distance from each of many points to the nearest face of a triangle mesh (or point of
// a cloud: faces (i, i, i)) over a uniform grid, and stratified surface sampling.  include/mnerf.h states the contract (the one
// distance formula, every float32 operation in its order, the key, the grid, the shells, the sampler and its integer mix);
// tests/geometry_ref.py restates it in NumPy, every query against every face.
//   grid_count  a thread a face: the number of cells its axis-aligned box overlaps
//   grid_fill   a thread a face: (cell, face) pairs from the face's own offset (the caller's scan of the counts): no atomics, and
//               the list, stably sorted by cell by the caller, is the same in every run
//   distance    a thread a query: Chebyshev shells of cells around the query's (clamped) cell, every face of every cell, the
//               minimum of (bits(d2) << 32 | face) in a register.  The caller sorts the queries by cell, so the lanes of a wave
//               walk the same cells and read the same pairs, faces and corners (one address across the lanes, or neighbours).
//   face_areas, sample   float64 areas; a thread a sample: binary search in the running sum, barycentrics from a 32-bit mix
// No atomics anywhere and no floating-point reduction across threads: two runs agree bit for bit, and the distance kernel's result
// is a minimum over a SET of faces, so it depends neither on the traversal nor on the grid, provided the stopping rule never
// leaves out a face that would have won.
//
// The stopping rule and its margin.  After shell r the faces not yet seen are registered in no cell of the cube K of shells <= r,
// so the cell box of such a face lies beyond K on some axis a and side; take the upper side: every point x of the face has
// cell(x_a) >= c_a + r + 1 (cell() does not decrease, and the face's box is made with the same function as the query's cell).
// Write G(v) for the COMPUTED (v - origin_a) / cell and X(v) for its real value: two roundings, |G - X| <= 2.0001 u |X|, u = 2^-24.
// From G(x_a) >= c_a + r + 1 and G(q_a) = c_a + fr_a:  X(x_a) - X(q_a) >= (r + 1 - fr_a) - 2.0001 u (G(x_a) + G(q_a)), and both G lie
// below dims_a <= 2^10, so the real gap is at least (r + 1 - fr_a) - 2^-12 cells (the lower side likewise with fr_a).  The sides of
// K that lie at or beyond the grid's own ends have no face behind them and are left out of the minimum m.  For a query outside the
// box [origin, hi] the gap is taken from q, the query clamped into the box: x_a lies in [origin_a, hi_a], so |x_a - p_a| =
// ex_a + |x_a - q_a| on the axes where p is outside and |x_b - p_b| >= ex_b on all of them, hence |x - p|^2 >= out2 + gap^2.
// That bounds the TRUE distance; the key holds the COMPUTED d2 of a face, which for a well-conditioned face differs from the true
// one by rounding: relatively by a few u where the distance is of the size of |p - a| (no cancellation), and absolutely, in the
// distance, by a few u (|p - a| + the face's size) where the plane term cancels, which inside and near the grid is at most
// C u sqrt(3) 2^10 cells = C 2^-13.2 cells.  MNR_MESHDIST_MARGIN = 2^-5 of a cell covers 2^-12 + C 2^-13.2 for C up to 300 and the
// roundings of (float(r) + m) and of the product with cell; MNR_MESHDIST_SHRINK = 1 - 2^-16 covers the relative part (C u for C up to
// 256), which matters for a query many box sizes away, where out2 dominates.  The cost is a thirty-second of a cell of pruning.
// What the margin does NOT cover is the LIMIT of include/mnerf.h (a sliver whose normal is rounding noise can compute a d2 far below
// its true distance): such a face is found when it lies in a visited cell and not otherwise.  tests/test_gpu_geometry.py holds
// the rule: automatic, single-cell, fine and flat grids against the brute-force restatement, bit for bit.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define MD_THREADS 256
#define MD_NONE 0x7f800000ffffffffull                       // (bits(+inf) << 32) | all ones: d2 = +inf, face = -1

// cell(v) of include/mnerf.h as a float (fmaxf(NaN, 0) = 0)
__host__ __device__ __forceinline__ float md_cell(float v, float origin, float cell, int dim) {
  return fminf(fmaxf(floorf((v - origin) / cell), 0.f), (float)(dim - 1));
}

// the cell box of a valid face; lo, hi [3]
__device__ __forceinline__ void md_box(const mnr_meshdist_args& g, const float* a, const float* b, const float* c, int* lo, int* hi) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = (int)md_cell(fminf(fminf(a[d], b[d]), c[d]), g.origin[d], g.cell, g.dims[d]);
    hi[d] = (int)md_cell(fmaxf(fmaxf(a[d], b[d]), c[d]), g.origin[d], g.cell, g.dims[d]);
  }
}

__global__ __launch_bounds__(MD_THREADS) void meshdist_count_kernel(mnr_meshdist_args g, int64_t* __restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (f >= g.n_faces) return;
  float a[3], b[3], c[3];
  int64_t n = 0;
  if (md_load(g.verts, g.n_verts, g.faces, f, a, b, c)) {
    int lo[3], hi[3];
    md_box(g, a, b, c, lo, hi);
    n = (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
  }
  counts[f] = n;
}

__global__ __launch_bounds__(MD_THREADS) void meshdist_fill_kernel(mnr_meshdist_args g, const int64_t* __restrict__ offsets, int64_t n_pairs,
                                                                   int* __restrict__ pair_cell, int* __restrict__ pair_face) {
  const int64_t f = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (f >= g.n_faces) return;
  float a[3], b[3], c[3];
  if (!md_load(g.verts, g.n_verts, g.faces, f, a, b, c)) return;
  int64_t at = offsets[f];
  const int64_t end = min(offsets[f + 1], n_pairs);
  if (at < 0) return;
  int lo[3], hi[3];
  md_box(g, a, b, c, lo, hi);
  for (int x = lo[0]; x <= hi[0]; ++x) {
    for (int y = lo[1]; y <= hi[1]; ++y) {
      for (int z = lo[2]; z <= hi[2]; ++z) {
        if (at >= end) return;
        pair_cell[at] = (int)(((int64_t)x * g.dims[1] + y) * g.dims[2] + z);
        pair_face[at] = (int)f;
        ++at;
      }
    }
  }
}

// every face of cell (x, y, z), which lies inside the grid, against the query
__device__ __forceinline__ void md_visit(const mnr_meshdist_args& g, const int64_t* __restrict__ cell_start, const int* __restrict__ pair_face,
                                         int64_t n_pairs, int x, int y, int z, const float* p, float lim, unsigned long long& best) {
  const int64_t at = ((int64_t)x * g.dims[1] + y) * g.dims[2] + z;
  const int64_t s = cell_start[at], e = cell_start[at + 1];
  if (s < 0 || e > n_pairs) return;
  for (int64_t i = s; i < e; ++i) {
    const int64_t f = pair_face[i];
    float a[3], b[3], c[3];
    if (f < 0 || f >= g.n_faces || !md_load(g.verts, g.n_verts, g.faces, f, a, b, c)) continue;
    const float d2 = md_d2(p, a, b, c);
    if (d2 <= lim) {
      const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, d2) << 32) | (unsigned long long)(unsigned)f;
      best = key < best ? key : best;
    }
  }
}

__global__ __launch_bounds__(MD_THREADS) void meshdist_query_kernel(mnr_meshdist_args g, const int64_t* __restrict__ cell_start,
                                                                    const int* __restrict__ pair_face, int64_t n_pairs,
                                                                    const float* __restrict__ points, const int64_t* __restrict__ order, int64_t n,
                                                                    float lim, float* __restrict__ d2, int* __restrict__ face,
                                                                    int* __restrict__ shells) {
  const int64_t t = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (t >= n) return;
  const int64_t q = order ? order[t] : t;
  if (q < 0 || q >= n) return;
  const float p[3] = {points[3 * q], points[3 * q + 1], points[3 * q + 2]};
  unsigned long long best = MD_NONE;
  int walked = 0;
  if (n_pairs > 0 && mesh_finite(p[0]) && mesh_finite(p[1]) && mesh_finite(p[2])) {
    int c[3];
    float fr[3], ex[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float qd = fminf(fmaxf(p[d], g.origin[d]), g.hi[d]);
      const float gd = (qd - g.origin[d]) / g.cell;
      const float cf = fminf(fmaxf(floorf(gd), 0.f), (float)(g.dims[d] - 1));
      c[d] = (int)cf;
      fr[d] = fminf(fmaxf(gd - cf, 0.f), 1.f);
      ex[d] = fmaxf(fmaxf(g.origin[d] - p[d], p[d] - g.hi[d]), 0.f);
    }
    const float out2 = mesh_dot(ex, ex);
    for (int r = 0;; ++r) {
      const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.dims[0] - 1);
      const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.dims[1] - 1);
      const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.dims[2] - 1);
      for (int x = x0; x <= x1; ++x) {
        const bool on_x = x - c[0] == r || c[0] - x == r;
        for (int y = y0; y <= y1; ++y) {
          if (on_x || y - c[1] == r || c[1] - y == r) {
            for (int z = z0; z <= z1; ++z) md_visit(g, cell_start, pair_face, n_pairs, x, y, z, p, lim, best);
          } else {                                           // the two caps of the shell (r > 0 here)
            if (c[2] - r >= 0) md_visit(g, cell_start, pair_face, n_pairs, x, y, c[2] - r, p, lim, best);
            if (c[2] + r <= g.dims[2] - 1) md_visit(g, cell_start, pair_face, n_pairs, x, y, c[2] + r, p, lim, best);
          }
        }
      }
      ++walked;
      bool open = false;
      float m = 1.f;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (c[d] - r > 0) open = true, m = fminf(m, fr[d]);
        if (c[d] + r < g.dims[d] - 1) open = true, m = fminf(m, 1.f - fr[d]);
      }
      if (!open) break;                                     // the shells have left the grid on every side
      const float bound = g.cell * fmaxf(((float)r + m) - MNR_MESHDIST_MARGIN, 0.f);
      const float lb2 = (out2 + bound * bound) * MNR_MESHDIST_SHRINK;
      if (__builtin_bit_cast(float, (unsigned)(best >> 32)) < lb2 || lb2 > lim) break;
    }
  }
  d2[q] = __builtin_bit_cast(float, (unsigned)(best >> 32));
  face[q] = (int)(unsigned)(best & 0xffffffffull);
  if (shells) shells[q] = walked;
}

__global__ __launch_bounds__(MD_THREADS) void meshdist_areas_kernel(const float* __restrict__ verts, int64_t n_verts, const int* __restrict__ faces,
                                                                    int64_t n_faces, double* __restrict__ area) {
  const int64_t f = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (f >= n_faces) return;
  float a[3], b[3], c[3];
  double out = 0.;
  if (md_load(verts, n_verts, faces, f, a, b, c)) {
    double u[3], v[3], n[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      u[d] = (double)b[d] - (double)a[d];
      v[d] = (double)c[d] - (double)a[d];
    }
    mesh_cross(u, v, n);
    out = 0.5 * sqrt(mesh_dot(n, n));
  }
  area[f] = out;
}

__host__ __device__ __forceinline__ uint32_t md_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(MD_THREADS) void meshdist_sample_kernel(const float* __restrict__ verts, int64_t n_verts, const int* __restrict__ faces,
                                                                     int64_t n_faces, const double* __restrict__ cum, int64_t n, uint32_t seed,
                                                                     float* __restrict__ points, int* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * MD_THREADS + threadIdx.x;
  if (i >= n) return;
  const double u = (((double)i + 0.5) / (double)n) * cum[n_faces - 1];
  int64_t lo = 0, hi = n_faces - 1;
  while (lo < hi) {                                          // the first k with cum[k] > u
    const int64_t mid = lo + (hi - lo) / 2;
    if (cum[mid] > u) hi = mid; else lo = mid + 1;
  }
  const uint32_t s = md_mix(seed);
  const uint32_t h1 = md_mix(s + 2u * (uint32_t)i), h2 = md_mix(s + (2u * (uint32_t)i + 1u));
  float r1 = (float)(h1 >> 8) * 5.9604644775390625e-08f, r2 = (float)(h2 >> 8) * 5.9604644775390625e-08f;
  if (r1 > 1.f - r2) r1 = 1.f - r1, r2 = 1.f - r2;
  const float b0 = (1.f - r1) - r2;
  float a[3], b[3], c[3];
  const bool ok = md_load(verts, n_verts, faces, lo, a, b, c);
#pragma unroll
  for (int d = 0; d < 3; ++d) points[3 * i + d] = ok ? (b0 * a[d] + r1 * b[d]) + r2 * c[d] : 0.f;
  face[i] = ok ? (int)lo : -1;
}

static int md_check_grid(const char* name, const mnr_meshdist_args* g) {
  MNR_CHECK_ARG(g, "%s: needs its arguments", name);
  const int st = md_check_mesh(name, g->verts, g->n_verts, g->faces, g->n_faces);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(g->cell > 0.f && g->cell <= MNR_F32_MAX, "%s: cell = %g must be positive and finite", name, (double)g->cell);
  for (int d = 0; d < 3; ++d) {
    MNR_CHECK_ARG(mesh_finite(g->origin[d]) && mesh_finite(g->hi[d]) && g->origin[d] <= g->hi[d],
                  "%s: origin and hi must be finite with origin <= hi, are %g and %g on axis %d", name, (double)g->origin[d], (double)g->hi[d], d);
    MNR_CHECK_ARG(g->dims[d] >= 1 && g->dims[d] <= MNR_MESHDIST_MAX_DIM, "%s: dims[%d] = %d must lie in 1 .. %d", name, d, g->dims[d],
                  MNR_MESHDIST_MAX_DIM);
  }
  return MNR_OK;
}

extern "C" int mnr_mesh_grid_count(const mnr_meshdist_args* g, int64_t* counts, void* stream) {
  const int st = md_check_grid("mnr_mesh_grid_count", g);
  if (st != MNR_OK) return st;
  if (g->n_faces == 0) return MNR_OK;
  MNR_CHECK_ARG(counts, "mnr_mesh_grid_count: needs counts [n_faces]");
  hipLaunchKernelGGL(meshdist_count_kernel, dim3((unsigned)mnr_cdiv(g->n_faces, MD_THREADS)), dim3(MD_THREADS), 0, (hipStream_t)stream, *g, counts);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mesh_grid_fill(const mnr_meshdist_args* g, const int64_t* offsets, int64_t n_pairs, int* pair_cell, int* pair_face,
                                  void* stream) {
  const int st = md_check_grid("mnr_mesh_grid_fill", g);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(n_pairs >= 0 && n_pairs < (1ll << 31), "mnr_mesh_grid_fill: n_pairs = %lld must lie in 0 .. 2^31 - 1", (long long)n_pairs);
  if (g->n_faces == 0 || n_pairs == 0) return MNR_OK;
  MNR_CHECK_ARG(offsets && pair_cell && pair_face, "mnr_mesh_grid_fill: needs offsets [n_faces + 1], pair_cell and pair_face [n_pairs]");
  hipLaunchKernelGGL(meshdist_fill_kernel, dim3((unsigned)mnr_cdiv(g->n_faces, MD_THREADS)), dim3(MD_THREADS), 0, (hipStream_t)stream, *g, offsets,
                     n_pairs, pair_cell, pair_face);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mesh_distance(const mnr_meshdist_args* g, const int64_t* cell_start, const int* pair_face, int64_t n_pairs,
                                 const float* points, const int64_t* order, int64_t n, float max_dist, float* d2, int* face, int* shells,
                                 void* stream) {
  const int st = md_check_grid("mnr_mesh_distance", g);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(max_dist > 0.f, "mnr_mesh_distance: max_dist = %g must be positive (+inf: no limit)", (double)max_dist);
  MNR_CHECK_ARG(n >= 0 && n_pairs >= 0 && n_pairs < (1ll << 31), "mnr_mesh_distance: n = %lld, n_pairs = %lld: n_pairs must lie in 0 .. 2^31 - 1",
                (long long)n, (long long)n_pairs);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(points && d2 && face, "mnr_mesh_distance: needs points [n,3], d2 [n] and face [n]");
  MNR_CHECK_ARG(n_pairs == 0 || (cell_start && pair_face), "mnr_mesh_distance: needs cell_start [cells + 1] and pair_face [n_pairs]");
  hipLaunchKernelGGL(meshdist_query_kernel, dim3((unsigned)mnr_cdiv(n, MD_THREADS)), dim3(MD_THREADS), 0, (hipStream_t)stream, *g, cell_start,
                     pair_face, n_pairs, points, order, n, max_dist * max_dist, d2, face, shells);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mesh_face_areas(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, double* area, void* stream) {
  const int st = md_check_mesh("mnr_mesh_face_areas", verts, n_verts, faces, n_faces);
  if (st != MNR_OK) return st;
  if (n_faces == 0) return MNR_OK;
  MNR_CHECK_ARG(area, "mnr_mesh_face_areas: needs area [n_faces]");
  hipLaunchKernelGGL(meshdist_areas_kernel, dim3((unsigned)mnr_cdiv(n_faces, MD_THREADS)), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, n_verts,
                     faces, n_faces, area);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mesh_sample(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, const double* cum, int64_t n,
                               uint32_t seed, float* points, int* face, void* stream) {
  const int st = md_check_mesh("mnr_mesh_sample", verts, n_verts, faces, n_faces);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(n >= 0 && n < (1ll << 31), "mnr_mesh_sample: n = %lld must lie in 0 .. 2^31 - 1", (long long)n);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(n_faces > 0 && cum && points && face, "mnr_mesh_sample: needs at least one face, cum [n_faces], points [n,3] and face [n]");
  hipLaunchKernelGGL(meshdist_sample_kernel, dim3((unsigned)mnr_cdiv(n, MD_THREADS)), dim3(MD_THREADS), 0, (hipStream_t)stream, verts, n_verts,
                     faces, n_faces, cum, n, seed, points, face);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
