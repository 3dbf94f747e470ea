// Marching tetrahedra on a regular grid, on device (gfx950): a density field -> an indexed triangle mesh.
//
// Grid.  field [nx, ny, nz] float32, field[i, j, k] at origin + spacing (i, j, k), linear point index p = (i ny + j) nz + k
// (64-bit).  A point is inside iff field >= level, so a NaN is outside.
//
// Decomposition (Kuhn / Freudenthal).  The cell with low corner p is cut into 6 tetrahedra, one per permutation (a, b, c) of
// the axes, in lexicographic order: corners p0 = p, p1 = p0 + e_a, p2 = p1 + e_b, p3 = p + (1, 1, 1).  Neighbouring cells cut
// their shared face along the same diagonal, so the mesh is watertight, and no case table is needed beyond the 16 sign
// patterns of ONE tetrahedron (mt_case below, worked out at compile time).  Every tetrahedron edge leaves its lower end in
// one of 7 directions, numbered (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1); it exists iff its upper end
// is in the grid and carries a vertex iff its ends differ in inside-ness.
//
// Vertex ids.  Vertices are ordered by the lower end's linear index, then by direction.  Per point one uint8 edge mask (bit e:
// edge e carries a vertex) and one int32 base id; the id of edge (p, e) is base[p] + popcount(mask[p] & ((1 << e) - 1)).
// 5 bytes a point, no hashing, no welding.
//
// Passes.  A workgroup of 256 threads owns the 256 consecutive linear indices [256 b, 256 b + 256), one a thread.
//   mt_classify_kernel       the mask of every point, and per workgroup the pair (vertices, triangles) it will emit
//   (host)                   the exclusive scan of those pairs, and the totals that size the outputs
//   mt_emit_vertices_kernel  base, positions, normals
//   mt_emit_faces_kernel     faces [T, 3] int32, ordered by cell, then tetrahedron, then triangle
// Inside a workgroup the exclusive prefix of the per-thread counts (0..7 vertices, 0..12 triangles) is taken bit plane by bit
// plane: __ballot of the plane, __popcll of the lanes below, and the 4 wave totals through LDS.  No atomics anywhere: two runs
// agree bit for bit, order included.
//
// Arithmetic: float32 in the order written (contraction off), so that a NumPy float32 restatement reproduces the positions
// bit for bit.  t = (level - f0) / (f1 - f0) lies in [0, 1] for finite ends (float subtraction is monotone); where it does not
// (a NaN or an infinity at one end) the vertex sits at t = 0.5.  Normal: the field gradient at the two ends (central
// differences, one-sided at the grid faces), interpolated with t; -g / |g|, and 0 where |g| is 0 or not finite.
//
// Faces.  With the corners' inside bits as a 4-bit pattern over the path positions 0..3: 1 or 3 inside: one triangle over the
// three edges at the lone corner l (the other ends ascending); 2 inside (a < b inside, c < d outside): the quad v(a,c), v(a,d),
// v(b,d), v(b,c) split along q0-q2.  Seen from outside (the low-field side) the listed order is counter-clockwise iff
//   sign(a, b, c) * (-1)^l > 0 (one inside), < 0 (three inside),   sign(a, b, c) * sign of (a, b, c, d) as a permutation > 0 (two),
// because det(p1 - p0, p2 - p0, p3 - p0) = det(e_a, e_b, e_c); otherwise each triangle is written with its last two ids swapped.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define MT_THREADS 256
#define MT_WAVES (MT_THREADS / 64)

// direction bits (x = 1, y = 2, z = 4) -> edge number
#define MT_DIR2E(d) ((0x65423100u >> (4 * (d))) & 7u)

// One tetrahedron's sign pattern m (bit r: path corner r is inside) -> packed case:
//   bits 0-1 triangles, bit 2 flip (before the permutation's parity), bits 4.. four vertices as (lower, upper) path positions, 2 + 2 bits each
static constexpr unsigned mt_case(unsigned m) {
  int n = 0;
  for (int r = 0; r < 4; ++r) n += (m >> r) & 1;
  if (n == 0 || n == 4) return 0;
  unsigned v[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
  unsigned ntri = 1, flip = 0;
  if (n == 1 || n == 3) {
    unsigned l = 0;
    for (unsigned r = 0; r < 4; ++r)
      if ((((m >> r) & 1) == 1) == (n == 1)) l = r;
    int k = 0;
    for (unsigned r = 0; r < 4; ++r) {
      if (r == l) continue;
      v[k][0] = r < l ? r : l;
      v[k][1] = r < l ? l : r;
      ++k;
    }
    flip = (l & 1) ^ (n == 3 ? 1u : 0u);
  } else {
    unsigned in[2] = {0, 0}, out[2] = {0, 0};
    int ki = 0, ko = 0;
    for (unsigned r = 0; r < 4; ++r) {
      if ((m >> r) & 1) in[ki++] = r; else out[ko++] = r;
    }
    const unsigned q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
    for (int k = 0; k < 4; ++k) {
      v[k][0] = q[k][0] < q[k][1] ? q[k][0] : q[k][1];
      v[k][1] = q[k][0] < q[k][1] ? q[k][1] : q[k][0];
    }
    const unsigned s[4] = {in[0], in[1], out[0], out[1]};
    unsigned inv = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i + 1; j < 4; ++j) inv += s[i] > s[j] ? 1u : 0u;
    flip = inv & 1;
    ntri = 2;
  }
  unsigned c = ntri | (flip << 2);
  for (int k = 0; k < 4; ++k) c |= (v[k][0] | (v[k][1] << 2)) << (4 + 4 * k);
  return c;
}

struct mt_cases {
  unsigned c[16];
};
static constexpr mt_cases MT_CASES = {{mt_case(0), mt_case(1), mt_case(2), mt_case(3), mt_case(4), mt_case(5), mt_case(6), mt_case(7),
                                       mt_case(8), mt_case(9), mt_case(10), mt_case(11), mt_case(12), mt_case(13), mt_case(14), mt_case(15)}};

// the 6 tetrahedra of a cell, lexicographic in (a, b, c): corner ids (bit 0 x, bit 1 y, bit 2 z) of p1 and p2, and the parity of (a, b, c)
#define MT_TET_C1(s) ((0x442211u >> (4 * (s))) & 7u)
#define MT_TET_C2(s) ((0x656353u >> (4 * (s))) & 7u)
#define MT_TET_ODD(s) ((0x26u >> (s)) & 1u)

struct mt_point {
  int64_t p;
  int i, j, k;
  bool valid;
};

__device__ __forceinline__ mt_point mt_my_point(const mnr_mt_args& a, int64_t n_points) {
  mt_point q;
  q.p = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  q.valid = q.p < n_points;
  const int64_t p = q.valid ? q.p : 0;
  if (n_points < (1ll << 31)) {                             // (the same for every thread: 32-bit divisions where they suffice)
    const unsigned p32 = (unsigned)p, ij = p32 / (unsigned)a.nz;
    q.k = (int)(p32 - ij * (unsigned)a.nz);
    q.i = (int)(ij / (unsigned)a.ny);
    q.j = (int)(ij - (unsigned)q.i * (unsigned)a.ny);
  } else {
    const int64_t ij = p / a.nz;
    q.k = (int)(p - ij * a.nz);
    q.i = (int)(ij / a.ny);
    q.j = (int)(ij - (int64_t)q.i * a.ny);
  }
  return q;
}

__device__ __forceinline__ int64_t mt_corner_offset(const mnr_mt_args& a, unsigned c) {
  return (int64_t)(c & 1) * a.ny * a.nz + (int64_t)((c >> 1) & 1) * a.nz + (int64_t)((c >> 2) & 1);
}

// triangles of the cell whose 8 corners have the inside bits cb (bit c: corner c)
__device__ __forceinline__ int mt_cell_triangles(unsigned cb) {
  if (cb == 0 || cb == 255) return 0;
  int n = 0;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const unsigned m = (cb & 1) | (((cb >> MT_TET_C1(s)) & 1) << 1) | (((cb >> MT_TET_C2(s)) & 1) << 2) | (((cb >> 7) & 1) << 3);
    n += (int)(MT_CASES.c[m] & 3);
  }
  return n;
}

// exclusive prefix of v (0 <= v < 2^BITS) over the workgroup in thread order; *total = the workgroup's sum (all threads call)
template <int BITS>
__device__ __forceinline__ int mt_block_prefix(int v, int* l_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int pre = 0, sum = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const unsigned long long bal = __ballot((v >> b) & 1);
    pre += __popcll(bal & below) << b;
    sum += __popcll(bal) << b;
  }
  __syncthreads();                                          // (l_w may still be read from the previous call)
  if (lane == 0) l_w[wave] = sum;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < MT_WAVES; ++w) {
    const int s = l_w[w];
    if (w < wave) pre += s;
    t += s;
  }
  *total = t;
  return pre;
}

__global__ __launch_bounds__(MT_THREADS) void mt_classify_kernel(mnr_mt_args a, int64_t n_points) {
  __shared__ int l_w[MT_WAVES];
  const mt_point q = mt_my_point(a, n_points);
  unsigned mask = 0;
  int ntri = 0;
  if (q.valid) {
    const bool ex = q.i + 1 < a.nx, ey = q.j + 1 < a.ny, ez = q.k + 1 < a.nz;
    unsigned cb = 0;
#pragma unroll
    for (unsigned c = 0; c < 8; ++c) {
      const bool there = (!(c & 1) || ex) && (!(c & 2) || ey) && (!(c & 4) || ez);
      if (there && a.field[q.p + mt_corner_offset(a, c)] >= a.level) cb |= 1u << c;
    }
    const unsigned in0 = cb & 1;
#pragma unroll
    for (unsigned c = 1; c < 8; ++c) {
      const bool there = (!(c & 1) || ex) && (!(c & 2) || ey) && (!(c & 4) || ez);
      if (there && ((cb >> c) & 1) != in0) mask |= 1u << MT_DIR2E(c);
    }
    if (ex && ey && ez) ntri = mt_cell_triangles(cb);
    a.mask[q.p] = (unsigned char)mask;
  }
  int nv_total, nt_total;
  (void)mt_block_prefix<3>(__builtin_popcount(mask), l_w, &nv_total);
  (void)mt_block_prefix<4>(ntri, l_w, &nt_total);
  if (threadIdx.x == 0) {
    a.counts[2 * (int64_t)blockIdx.x] = nv_total;
    a.counts[2 * (int64_t)blockIdx.x + 1] = nt_total;
  }
}

// the field gradient at grid point (i, j, k): (f[hi] - f[lo]) / (spacing (hi - lo)) per axis, hi / lo the neighbours clipped to the grid
__device__ __forceinline__ void mt_gradient(const mnr_mt_args& a, int i, int j, int k, float* g) {
  const int idx[3] = {i, j, k}, n[3] = {a.nx, a.ny, a.nz};
  const int64_t stride[3] = {(int64_t)a.ny * a.nz, (int64_t)a.nz, 1};
  const int64_t p = ((int64_t)i * a.ny + j) * a.nz + k;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int lo = idx[d] > 0 ? idx[d] - 1 : 0, hi = idx[d] + 1 < n[d] ? idx[d] + 1 : n[d] - 1;
    const float fl = a.field[p + (int64_t)(lo - idx[d]) * stride[d]], fh = a.field[p + (int64_t)(hi - idx[d]) * stride[d]];
    g[d] = (fh - fl) / (a.spacing * (float)(hi - lo));
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_emit_vertices_kernel(mnr_mt_args a, int64_t n_points) {
  __shared__ int l_w[MT_WAVES];
  const mt_point q = mt_my_point(a, n_points);
  unsigned mask = 0;
  if (q.valid) {
    // (bits of edges that leave the grid are never set by the classification; a mask that is not this grid's must not make a read leave it)
    const unsigned ex = q.i + 1 < a.nx ? 1u : 0u, ey = q.j + 1 < a.ny ? 1u : 0u, ez = q.k + 1 < a.nz ? 1u : 0u;
    const unsigned in_grid = ex | (ey << 1) | (ez << 2) | ((ex & ey) << 3) | ((ex & ez) << 4) | ((ey & ez) << 5) | ((ex & ey & ez) << 6);
    mask = a.mask[q.p] & in_grid;
  }
  int total;
  const int pre = mt_block_prefix<3>(__builtin_popcount(mask), l_w, &total);
  if (!q.valid) return;
  int64_t id = a.offsets[2 * (int64_t)blockIdx.x] + pre;
  a.base[q.p] = (int)id;
  if (mask == 0) return;
  const float f0 = a.field[q.p];
  const int i0[3] = {q.i, q.j, q.k};
  float P0[3], g0[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) P0[d] = a.origin[d] + a.spacing * (float)i0[d];
  mt_gradient(a, q.i, q.j, q.k, g0);
  for (unsigned e = 0; e < 7; ++e) {
    if (!((mask >> e) & 1)) continue;
    const unsigned c = (0x7653421u >> (4 * e)) & 7u;        // edge number -> direction bits
    if (id >= a.n_verts) return;                            // (a mask that is not this field's: never write past the outputs)
    const int i1[3] = {q.i + (int)(c & 1), q.j + (int)((c >> 1) & 1), q.k + (int)((c >> 2) & 1)};
    const float f1 = a.field[q.p + mt_corner_offset(a, c)];
    float t = (a.level - f0) / (f1 - f0);
    if (!(t >= 0.f && t <= 1.f)) t = 0.5f;
    float g1[3], g[3];
    mt_gradient(a, i1[0], i1[1], i1[2], g1);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float P1 = a.origin[d] + a.spacing * (float)i1[d];
      a.verts[id * 3 + d] = P0[d] + t * (P1 - P0[d]);
      g[d] = g0[d] + t * (g1[d] - g0[d]);
    }
    const float len = sqrtf(mesh_dot(g, g));
    const bool ok = len > 0.f && len <= MNR_F32_MAX;
#pragma unroll
    for (int d = 0; d < 3; ++d) a.normals[id * 3 + d] = ok ? -g[d] / len : 0.f;
    ++id;
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_emit_faces_kernel(mnr_mt_args a, int64_t n_points) {
  __shared__ int l_w[MT_WAVES];
  const mt_point q = mt_my_point(a, n_points);
  unsigned cb = 0;
  int ntri = 0;
  if (q.valid && q.i + 1 < a.nx && q.j + 1 < a.ny && q.k + 1 < a.nz) {
    // a cell has all 7 edges, so its corners' bits follow from its own point and its mask
    const unsigned mask = a.mask[q.p];
    if (mask != 0) {
      const unsigned in0 = a.field[q.p] >= a.level ? 1u : 0u;
      cb = in0;
#pragma unroll
      for (unsigned c = 1; c < 8; ++c) cb |= (in0 ^ ((mask >> MT_DIR2E(c)) & 1)) << c;
      ntri = mt_cell_triangles(cb);
    }
  }
  int total;
  const int pre = mt_block_prefix<4>(ntri, l_w, &total);
  if (ntri == 0) return;
  int64_t tri = a.offsets[2 * (int64_t)blockIdx.x + 1] + pre;
  for (int s = 0; s < 6; ++s) {
    const unsigned corner[4] = {0u, MT_TET_C1(s), MT_TET_C2(s), 7u};
    const unsigned m = (cb & 1) | (((cb >> corner[1]) & 1) << 1) | (((cb >> corner[2]) & 1) << 2) | (((cb >> 7) & 1) << 3);
    const unsigned cs = MT_CASES.c[m];
    const int nt = (int)(cs & 3);
    if (nt == 0) continue;
    const bool flip = (((cs >> 2) & 1) ^ MT_TET_ODD(s)) != 0;
    int v[4] = {0, 0, 0, 0};
    for (int r = 0; r < nt + 2; ++r) {
      const unsigned lo = (cs >> (4 + 4 * r)) & 3, hi = (cs >> (6 + 4 * r)) & 3;
      const unsigned c_lo = lo == 0 ? corner[0] : (lo == 1 ? corner[1] : corner[2]);        // (a lower end is never p3)
      const unsigned c_hi = hi == 1 ? corner[1] : (hi == 2 ? corner[2] : corner[3]);
      const int64_t pl = q.p + mt_corner_offset(a, c_lo);
      const unsigned e = MT_DIR2E(c_lo ^ c_hi);
      v[r] = a.base[pl] + __builtin_popcount((unsigned)a.mask[pl] & ((1u << e) - 1u));
    }
    for (int r = 0; r < nt; ++r) {
      if (tri >= a.n_faces) return;                         // (see mt_emit_vertices_kernel)
      const int v1 = v[r + 1], v2 = v[r + 2];
      a.faces[tri * 3] = v[0];
      a.faces[tri * 3 + 1] = flip ? v2 : v1;
      a.faces[tri * 3 + 2] = flip ? v1 : v2;
      ++tri;
    }
  }
}

extern "C" int64_t mnr_mt_workgroups(int64_t n_points) { return n_points > 0 ? (n_points + MT_THREADS - 1) / MT_THREADS : 0; }

static int mt_check_grid(const mnr_mt_args* a, const char* who, int64_t* n_points) {
  MNR_CHECK_ARG(a && a->field && a->mask, "%s: needs the field and the mask", who);
  MNR_CHECK_ARG(a->nx >= 2 && a->ny >= 2 && a->nz >= 2, "%s: every grid dimension must be at least 2, got [%d, %d, %d]", who, a->nx,
                a->ny, a->nz);
  *n_points = (int64_t)a->nx * a->ny * a->nz;
  MNR_CHECK_ARG(mnr_mt_workgroups(*n_points) < (1ll << 31), "%s: a grid of [%d, %d, %d] points is too large", who, a->nx, a->ny, a->nz);
  MNR_CHECK_ARG(a->spacing > 0.f && a->spacing <= MNR_F32_MAX, "%s: the spacing must be positive and finite, is %g", who,
                (double)a->spacing);
  for (int d = 0; d < 3; ++d)
    MNR_CHECK_ARG(mesh_finite(a->origin[d]), "%s: the origin must be finite", who);
  return MNR_OK;
}

extern "C" int mnr_mt_classify(const mnr_mt_args* a, void* stream) {
  int64_t n = 0;
  if (int st = mt_check_grid(a, "mnr_mt_classify", &n)) return st;
  MNR_CHECK_ARG(a->counts, "mnr_mt_classify: needs counts [workgroups, 2]");
  hipLaunchKernelGGL(mt_classify_kernel, dim3((unsigned)mnr_mt_workgroups(n)), dim3(MT_THREADS), 0, (hipStream_t)stream, *a, n);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mt_emit_vertices(const mnr_mt_args* a, void* stream) {
  int64_t n = 0;
  if (int st = mt_check_grid(a, "mnr_mt_emit_vertices", &n)) return st;
  MNR_CHECK_ARG(a->offsets && a->base, "mnr_mt_emit_vertices: needs the scanned offsets [workgroups, 2] and base [points]");
  MNR_CHECK_ARG(a->n_verts >= 0 && a->n_verts < (1ll << 31), "mnr_mt_emit_vertices: %lld vertices, must be below 2^31", (long long)a->n_verts);
  MNR_CHECK_ARG(a->n_verts == 0 || (a->verts && a->normals), "mnr_mt_emit_vertices: needs verts and normals [n_verts, 3]");
  hipLaunchKernelGGL(mt_emit_vertices_kernel, dim3((unsigned)mnr_mt_workgroups(n)), dim3(MT_THREADS), 0, (hipStream_t)stream, *a, n);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mt_emit_faces(const mnr_mt_args* a, void* stream) {
  int64_t n = 0;
  if (int st = mt_check_grid(a, "mnr_mt_emit_faces", &n)) return st;
  MNR_CHECK_ARG(a->offsets && a->base, "mnr_mt_emit_faces: needs the scanned offsets [workgroups, 2] and base [points]");
  MNR_CHECK_ARG(a->n_faces >= 0 && a->n_faces < (1ll << 31), "mnr_mt_emit_faces: %lld triangles, must be below 2^31", (long long)a->n_faces);
  MNR_CHECK_ARG(a->n_faces == 0 || a->faces, "mnr_mt_emit_faces: needs faces [n_faces, 3]");
  hipLaunchKernelGGL(mt_emit_faces_kernel, dim3((unsigned)mnr_mt_workgroups(n)), dim3(MT_THREADS), 0, (hipStream_t)stream, *a, n);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
