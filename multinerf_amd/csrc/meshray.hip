// Mesh ray casting on device (gfx950): the nearest intersection of each of many rays with a triangle mesh over the uniform grid of
// meshdist.hip (mnr_mesh_grid_count / mnr_mesh_grid_fill), and the shading of the hits.  include/mnerf.h states the contract (the one
// hit test, every operation in its order, the key, the walk); tests/raycast_ref.py restates the hit test in NumPy, every ray against
// every face, with no grid.
//   cast    a thread a ray: the slabs of cells along the ray's dominant axis, in each slab the rectangle of cells the ray can touch,
//           every face of every such cell, the minimum of (bits(t) << 32 | face) in a register.  The caller orders the rays (an 8 x 8
//           pixel tile a wave, or by entry cell) so that the lanes of a wave walk the same cells and read the same pairs and corners.
//   shade   a thread a ray: the colour and normal stage of raster.hip's shading pass on a given (face, bary).
// No atomics, no LDS and no reduction across threads.  The result is a minimum over a SET of faces, the faces that pass a hit test
// which knows the ray and the face and nothing else, so it depends neither on the grid nor on the traversal nor on the order of the
// rays, provided the walk never leaves out a face that would have won.
//
// The hit test (Woop, Benthin, Wald 2013) and what it is exact about.  The corners are translated to the ray origin and sheared so
// that the ray becomes the z axis: A' = (A_kx - Sx A_kz, A_ky - Sy A_kz), |Sx|, |Sy| <= 1.  That costs one rounding in a - o, one in S,
// one in the product and one in the difference: every sheared corner is off by at most 4 u M in each of its two coordinates, u = 2^-24,
// M the largest |corner - o| coordinate of the face.  The three edge functions are then evaluated in float64 from those float32
// numbers: a product of two float32 has 48 significant bits and is exact, the difference of two such products is rounded once and
// keeps its sign.  So the inside test is the EXACT answer for a triangle whose corners were moved by at most 4 sqrt(2) u M inside
// their planes of constant kz, however thin the triangle is: a ray that passes has a point within 6 u M of the true face, and two
// faces that share an edge see the very same two sheared corners, so the ray is on opposite sides of the edge or on it for both
// (zeros count as inside): never a crack.  The same exactness means that three collinear corners, whose sheared images are collinear
// to rounding only, are a sliver of some width to this test and can be hit by a ray aimed at them; two equal corners cannot (U, or V,
// or W is 0 and the other two cancel exactly).  So a face whose float64 normal vanishes is excluded by its own clause, evaluated only
// for a ray that has passed everything else.  t interpolates Az = Sz A_kz (two roundings) with the exact weights, rounded twice more:
// the point o + t d lies within 6 u M of the moved triangle along the dominant axis.  Together: a face that passes with parameter t
// has a true point Q with |Q - (o + t d)| <= 12 u M in the maximum norm.
//
// The walk and its margin.  R = 2 max_a max(|o_a|, |origin_a|, |hi_a|) bounds M for every face of the grid (its corners lie in
// [origin, hi]) and the magnitude of every coordinate the walk forms.  w = MNR_MESHRAY_MARGIN cell + MNR_MESHRAY_REL R is the margin in
// world units, wt = w |Sz| the same in the ray parameter.  A slab s is the cells with index s on the dominant axis kz.  For slab s the
// thread takes the parameter interval in which the ray's kz coordinate lies in [origin_kz + s cell - w, origin_kz + (s + 1) cell + w],
// clips it to [t_min, t_max], widens it by wt, evaluates the two other coordinates at its two ends from the ray equation itself
// (o_a + t d_a: nothing is carried from slab to slab, so no error accumulates), widens that interval by w and visits every cell whose
// index lies in the resulting rectangle (cell() of include/mnerf.h, clamped to the grid).
//   Claim: a face F that passes with parameter t_F in (t_min, t_max] is registered in a visited cell.  Let Q be its true point (above)
//   and s_Q = cell(Q_kz).  Q lies in F's box, so F is registered in the cell of Q.  P = o + t_F d has |P_kz - Q_kz| <= 12 u R, and
//   cell() as computed differs from the real quotient by at most 2^-12 of a cell (meshdist.hip argues it), so P_kz lies in slab s_Q's
//   widened range: t_F lies in the interval taken for s_Q.  The ends of that interval and the coordinates at them carry at most 8
//   roundings of numbers below R, 8 u R; Q_a is within 12 u R of P_a, and cell() adds its 2^-12 of a cell.  MNR_MESHRAY_REL = 2^-18 = 64 u
//   and MNR_MESHRAY_MARGIN = 2^-5 cover 12 + 8 and 2^-12 with room to spare, so cell(Q_a) lies in the rectangle on both axes.
//   Stopping: the slabs are walked in the ray's direction.  After slab s every face not yet seen has, by the claim, s_Q beyond s, so
//   Q_kz lies beyond the far plane of slab s but for 2^-12 of a cell, P_kz beyond it but for that and 12 u R, and t_F >= tn - wt for the
//   real parameter tn of that plane; the computed tn is within 5 u R |Sz| < wt of it.  The thread stops when best t < tn - 2 wt: no face
//   not yet seen can then have a key at or below the best one, equal t with a lower id included.
// The loop is bounded by construction: the slab index is an integer that moves by one an iteration, at most dims_kz <= 1024 times;
// the rectangle's indices are clamped into the grid before they are converted, so NaN and infinities in the floats (a parameter
// interval that overflows) can widen the visit and cannot leave the arrays.  Rays with a component that is not finite, d = 0 or a
// reciprocal 1 / d_kz that overflows return the empty result before the loop.  cell_start, pair_face, order and face entries outside
// their ranges are skipped as in mnr_mesh_distance.  tests/test_gpu_raycast.py holds the claim: automatic, single-cell, fine and coarse
// grids, permuted rays and a tile order against the brute-force restatement, bit for bit.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define MR_THREADS 256
#define MR_NONE 0x7f800000ffffffffull                       // (bits(+inf) << 32) | all ones: t = +inf, face = -1

__host__ __device__ __forceinline__ float mr_pick(const float* v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

struct mr_ray {
  float o[3];
  int kx, ky, kz;
  float Sx, Sy, Sz;
};

// the ray's shear; false: the ray has the empty result (a component that is not finite, d = 0, 1 / d_kz not finite)
__host__ __device__ __forceinline__ bool mr_setup(const float* o, const float* d, mr_ray& r) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.o[k] = o[k];
    ok = ok && mesh_finite(o[k]) && mesh_finite(d[k]);
  }
  const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
  int kz = 0;
  if (ay > ax) kz = 1;
  if (az > fmaxf(ax, ay)) kz = 2;                            // the lowest index among equal magnitudes
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dz = mr_pick(d, kz);
  if (dz < 0.f) {
    const int s = kx;
    kx = ky, ky = s;
  }
  r.kx = kx, r.ky = ky, r.kz = kz;
  r.Sx = mr_pick(d, kx) / dz;
  r.Sy = mr_pick(d, ky) / dz;
  r.Sz = 1.f / dz;
  return ok && dz != 0.f && mesh_finite(r.Sz);
}

// the hit test of include/mnerf.h; t and l [3] are written when it returns true
__host__ __device__ __forceinline__ bool mr_hit(const mr_ray& r, const float* a, const float* b, const float* c, int cull, float t_min,
                                                float t_max, float* t, float* l) {
  float A[3], B[3], C[3];
  mesh_sub(a, r.o, A);
  mesh_sub(b, r.o, B);
  mesh_sub(c, r.o, C);
  const float Ak = mr_pick(A, r.kz), Bk = mr_pick(B, r.kz), Ck = mr_pick(C, r.kz);
  const float Ax = mr_pick(A, r.kx) - r.Sx * Ak, Ay = mr_pick(A, r.ky) - r.Sy * Ak, Az = r.Sz * Ak;
  const float Bx = mr_pick(B, r.kx) - r.Sx * Bk, By = mr_pick(B, r.ky) - r.Sy * Bk, Bz = r.Sz * Bk;
  const float Cx = mr_pick(C, r.kx) - r.Sx * Ck, Cy = mr_pick(C, r.ky) - r.Sy * Ck, Cz = r.Sz * Ck;
  const double U = (double)Cx * (double)By - (double)Cy * (double)Bx;
  const double V = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
  const double W = (double)Bx * (double)Ay - (double)By * (double)Ax;
  if ((U < 0. || V < 0. || W < 0.) && (U > 0. || V > 0. || W > 0.)) return false;
  const double det = (U + V) + W;
  if (det == 0.) return false;
  if (cull == MNR_RASTER_CULL_BACK && !(det > 0.)) return false;
  const float tt = (float)(((U * (double)Az + V * (double)Bz) + W * (double)Cz) / det);
  if (!(tt > t_min && tt <= t_max && mesh_finite(tt))) return false;      // (a NaN fails here)
  double ab[3], ac[3], nn[3];                                 // a face without area: only a ray that passes so far pays for this
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = (double)b[k] - (double)a[k];
    ac[k] = (double)c[k] - (double)a[k];
  }
  mesh_cross(ab, ac, nn);
  if (nn[0] == 0. && nn[1] == 0. && nn[2] == 0.) return false;
  *t = tt;
  l[0] = (float)(U / det), l[1] = (float)(V / det), l[2] = (float)(W / det);
  return true;
}

// float grid coordinate -> an index inside [0, dim): NaN and -inf give 0, +inf gives dim - 1
__device__ __forceinline__ int mr_index(float g, int dim) { return (int)fminf(fmaxf(floorf(g), 0.f), (float)(dim - 1)); }

// every face of cell `at`, which lies inside the grid, against the ray
__device__ __forceinline__ void mr_visit(const mnr_meshdist_args& g, const int64_t* __restrict__ cell_start, const int* __restrict__ pair_face,
                                         int64_t n_pairs, int64_t at, const mr_ray& r, int cull, float t_min, float t_max,
                                         unsigned long long& best, float* bl) {
  const int64_t s = cell_start[at], e = cell_start[at + 1];
  if (s < 0 || e > n_pairs) return;
  for (int64_t i = s; i < e; ++i) {
    const int64_t f = pair_face[i];
    float a[3], b[3], c[3], t, l[3];
    if (f < 0 || f >= g.n_faces || !md_load(g.verts, g.n_verts, g.faces, f, a, b, c)) continue;
    if (!mr_hit(r, a, b, c, cull, t_min, t_max, &t, l)) continue;
    const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, t) << 32) | (unsigned long long)(unsigned)f;
    if (key < best) {
      best = key;
      bl[0] = l[0], bl[1] = l[1], bl[2] = l[2];
    }
  }
}

__global__ __launch_bounds__(MR_THREADS) void meshray_cast_kernel(mnr_meshdist_args g, const int64_t* __restrict__ cell_start,
                                                                  const int* __restrict__ pair_face, int64_t n_pairs,
                                                                  const float* __restrict__ origins, const float* __restrict__ directions,
                                                                  const int64_t* __restrict__ order, int64_t n, float t_min, float t_max, int cull,
                                                                  float* __restrict__ t_out, int* __restrict__ face, float* __restrict__ bary) {
  const int64_t tid = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (tid >= n) return;
  const int64_t q = order ? order[tid] : tid;
  if (q < 0 || q >= n) return;
  const float o[3] = {origins[3 * q], origins[3 * q + 1], origins[3 * q + 2]};
  const float d[3] = {directions[3 * q], directions[3 * q + 1], directions[3 * q + 2]};
  unsigned long long best = MR_NONE;
  float bl[3] = {0.f, 0.f, 0.f};
  mr_ray r;
  if (n_pairs > 0 && mr_setup(o, d, r)) {
    const int kz = r.kz;
    const float okz = mr_pick(o, kz), dkz = mr_pick(d, kz);
    const float gorg = mr_pick(g.origin, kz);
    const int dimz = kz == 0 ? g.dims[0] : (kz == 1 ? g.dims[1] : g.dims[2]);
    float R = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) R = fmaxf(R, fmaxf(fabsf(o[a]), fmaxf(fabsf(g.origin[a]), fabsf(g.hi[a]))));
    const float w = MNR_MESHRAY_MARGIN * g.cell + MNR_MESHRAY_REL * (2.f * R);
    const float wt = fminf(w * fabsf(r.Sz), MNR_F32_MAX);
    // the slabs the ray's kz coordinate crosses over [t_min, t_max]
    const float c0 = okz + t_min * dkz, c1 = okz + t_max * dkz;
    const float gl = ((fminf(c0, c1) - 2.f * w) - gorg) / g.cell, gh = ((fmaxf(c0, c1) + 2.f * w) - gorg) / g.cell;
    const bool some = gh >= 0.f && gl < (float)dimz;         // (a NaN: none)
    const int s0 = mr_index(gl, dimz), s1 = mr_index(gh, dimz);
    const int count = some ? s1 - s0 + 1 : 0;                // at most dimz <= MNR_MESHDIST_MAX_DIM
    const bool up = dkz > 0.f;
    const int ax2[2] = {r.kx, r.ky};
    for (int i = 0; i < count; ++i) {
      const int s = up ? s0 + i : s1 - i;
      const float zlo = (gorg + (float)s * g.cell) - w, zhi = (gorg + (float)(s + 1) * g.cell) + w;
      float ta = (zlo - okz) * r.Sz, tb = (zhi - okz) * r.Sz;
      if (!up) {
        const float x = ta;
        ta = tb, tb = x;
      }
      ta = fmaxf(ta, t_min) - wt;
      tb = fminf(tb, t_max) + wt;
      int lo[2], hi[2];
      bool any = true;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int a = ax2[j];
        const float oa = mr_pick(o, a), da = mr_pick(d, a), ga = mr_pick(g.origin, a);
        const int dim = a == 0 ? g.dims[0] : (a == 1 ? g.dims[1] : g.dims[2]);
        const float pa = da == 0.f ? oa : oa + ta * da, pb = da == 0.f ? oa : oa + tb * da;
        const float l0 = ((fminf(pa, pb) - w) - ga) / g.cell, h0 = ((fmaxf(pa, pb) + w) - ga) / g.cell;
        if ((h0 < 0.f) || (l0 >= (float)dim)) any = false;   // (a NaN skips nothing)
        lo[j] = mr_index(l0, dim), hi[j] = mr_index(h0, dim);
      }
      if (any) {
        for (int iu = lo[0]; iu <= hi[0]; ++iu) {
          for (int iv = lo[1]; iv <= hi[1]; ++iv) {
            const int x = kz == 0 ? s : (r.kx == 0 ? iu : iv);
            const int y = kz == 1 ? s : (r.kx == 1 ? iu : iv);
            const int z = kz == 2 ? s : (r.kx == 2 ? iu : iv);
            mr_visit(g, cell_start, pair_face, n_pairs, ((int64_t)x * g.dims[1] + y) * g.dims[2] + z, r, cull, t_min, t_max, best, bl);
          }
        }
      }
      const float zex = up ? gorg + (float)(s + 1) * g.cell : gorg + (float)s * g.cell;
      const float tn = (zex - okz) * r.Sz;
      if (__builtin_bit_cast(float, (unsigned)(best >> 32)) < tn - 2.f * wt) break;
    }
  }
  t_out[q] = __builtin_bit_cast(float, (unsigned)(best >> 32));
  face[q] = (int)(unsigned)(best & 0xffffffffull);
#pragma unroll
  for (int k = 0; k < 3; ++k) bary[3 * q + k] = bl[k];
}

__device__ __forceinline__ float mr_texel(const mnr_raster_args& a, int x, int y, int d) {
  const int64_t at = 3 * ((int64_t)y * a.Wt + x) + d;
  return a.texture_u8 ? (float)((const unsigned char*)a.texture)[at] / 255.f : ((const float*)a.texture)[at];
}

// the colour and normal stage of raster_shade_kernel (raster.hip), restated: equal (face, bary) give equal bits
__global__ __launch_bounds__(MR_THREADS) void meshray_shade_kernel(mnr_raster_args a, const int* __restrict__ face, const float* __restrict__ bary,
                                                                   int64_t n, float* __restrict__ normals, float* __restrict__ rgb) {
  const int64_t t = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (t >= n) return;
  const int64_t f = face[t];
  float nrm[3] = {0.f, 0.f, 0.f}, col[3] = {a.bg[0], a.bg[1], a.bg[2]};
  int id[3];
  if (f >= 0 && f < a.n_faces && mesh_face_ids(a.faces, f, a.n_verts, id)) {
    const float l[3] = {bary[3 * t], bary[3 * t + 1], bary[3 * t + 2]};
    float vn[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
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
        const float top = (1.f - fx) * mr_texel(a, xa, ya, d) + fx * mr_texel(a, xb, ya, d);
        const float bot = (1.f - fx) * mr_texel(a, xa, yb, d) + fx * mr_texel(a, xb, yb, d);
        col[d] = (1.f - fy) * top + fy * bot;
      }
    } else {
#pragma unroll
      for (int d = 0; d < 3; ++d) col[d] = 0.5f + 0.5f * nrm[d];
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    normals[3 * t + d] = nrm[d];
    rgb[3 * t + d] = col[d];
  }
}

extern "C" int mnr_mesh_raycast(const mnr_meshdist_args* g, const int64_t* cell_start, const int* pair_face, int64_t n_pairs,
                                const float* origins, const float* directions, const int64_t* order, int64_t n, float t_min, float t_max,
                                int cull, float* t, int* face, float* bary, void* stream) {
  const char* name = "mnr_mesh_raycast";
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
  MNR_CHECK_ARG(t_min >= 0.f && t_min <= MNR_F32_MAX && t_max > t_min, "%s: needs 0 <= t_min < t_max (+inf: no limit), are %g and %g", name,
                (double)t_min, (double)t_max);
  MNR_CHECK_ARG(cull == MNR_RASTER_CULL_NONE || cull == MNR_RASTER_CULL_BACK, "%s: cull = %d is neither NONE nor BACK", name, cull);
  MNR_CHECK_ARG(n >= 0 && n_pairs >= 0 && n_pairs < (1ll << 31), "%s: n = %lld, n_pairs = %lld: n_pairs must lie in 0 .. 2^31 - 1", name,
                (long long)n, (long long)n_pairs);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(origins && directions && t && face && bary, "%s: needs origins, directions [n,3], t, face [n] and bary [n,3]", name);
  MNR_CHECK_ARG(n_pairs == 0 || (cell_start && pair_face), "%s: needs cell_start [cells + 1] and pair_face [n_pairs]", name);
  hipLaunchKernelGGL(meshray_cast_kernel, dim3((unsigned)mnr_cdiv(n, MR_THREADS)), dim3(MR_THREADS), 0, (hipStream_t)stream, *g, cell_start,
                     pair_face, n_pairs, origins, directions, order, n, t_min, t_max, cull, t, face, bary);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_raycast_shade(const mnr_raster_args* a, const int* face, const float* bary, int64_t n, float* normals, float* rgb,
                                 void* stream) {
  const char* name = "mnr_raycast_shade";
  MNR_CHECK_ARG(a, "%s: needs its arguments", name);
  const int st = md_check_mesh(name, a->verts, a->n_verts, a->faces, a->n_faces);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(n >= 0, "%s: n = %lld must not be negative", name, (long long)n);
  MNR_CHECK_ARG(a->n_faces == 0 || a->n_verts == 0 || a->normals, "%s: needs normals [n_verts,3]", name);
  MNR_CHECK_ARG(!(a->colors && a->texture), "%s: colors and texture are both given: the colour has one source", name);
  MNR_CHECK_ARG(!a->texture || (a->uv && a->Ht >= 1 && a->Wt >= 1 && a->Ht <= (1 << 24) && a->Wt <= (1 << 24)),
                "%s: a texture needs uv [n_faces,3,2] and 1 .. 2^24 texels a side, has %d x %d", name, a->Ht, a->Wt);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(face && bary && normals && rgb, "%s: needs face [n] and bary, normals, rgb [n,3]", name);
  hipLaunchKernelGGL(meshray_shade_kernel, dim3((unsigned)mnr_cdiv(n, MR_THREADS)), dim3(MR_THREADS), 0, (hipStream_t)stream, *a, face, bary, n,
                     normals, rgb);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
