// Mesh registration on device (gfx950): what turns the nearest FACE of csrc/meshdist.hip into a correspondence and a set of
// correspondences into normal equations, and the polygonal crop volume.  include/mnerf.h states the contract ("Mesh
// registration"), tests/registration_ref.py restates it in NumPy.
//   closest       a thread a query: the closest point on the face mnr_mesh_distance returned and that face's unit normal, from
//                 the terms of the distance formula themselves, so that |p - x|^2 is the d2 that chose the face up to rounding
//   face_normals  a thread a face: the same normal expression
//   icp_sums      the 47 float64 sums of one ICP iteration (point-to-point and point-to-plane).  Two levels: workgroup b of B takes
//                 the queries b * 256 + t + k * B * 256 (a fixed assignment), every thread adds its own in ascending k, the 256
//                 threads' sums are added by a fixed tree in LDS (16 x 16), and one workgroup adds the B partials in four ascending
//                 runs and those in order.  No atomics: two runs agree bit for bit.
//   crop_polygon  a thread a point: even-odd crossing count against the polygon of a prism, float64; the polygon's address is
//                 the same in every lane, so its loads are scalar
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define MR_THREADS 256
#define MR_MAX_BLOCKS 256                                   // one workgroup a CU; the second stage then adds at most 256 partials an entry
#define MR_SUMS MNR_ICP_SUMS
#define MR_ROUND 16                                         // accumulators reduced per pass through LDS (47 -> 3 passes of 16)
#define MR_ACC (3 * MR_ROUND)

// t of seg(p, u, v) (include/mnerf.h, "Mesh geometry"): the operations of md_seg
__host__ __device__ __forceinline__ float mr_seg_t(const float* p, const float* u, const float* v) {
  float uv[3], up[3];
  mesh_sub(v, u, uv);
  mesh_sub(p, u, up);
  const float L = mesh_dot(uv, uv);
  float t = 0.f;
  if (L > 0.f) t = fminf(fmaxf(mesh_dot(up, uv) / L, 0.f), 1.f);
  return t;
}

// n / sqrt(nn), or 0 when nn is not positive and finite
__host__ __device__ __forceinline__ void mr_unit(const float* n, float nn, float* o) {
  const bool ok = nn > 0.f && nn <= MNR_F32_MAX;
  const float len = sqrtf(nn);
#pragma unroll
  for (int d = 0; d < 3; ++d) o[d] = ok ? n[d] / len : 0.f;
}

// the closest point of include/mnerf.h on the valid face (a, b, c) and the face's unit normal
__host__ __device__ __forceinline__ void mr_closest(const float* p, const float* a, const float* b, const float* c, float* x, float* nrm) {
  const float s_ab = md_seg(p, a, b), s_bc = md_seg(p, b, c), s_ca = md_seg(p, c, a);
  float best = s_ab;
  int k = 0;
  if (s_bc < best) best = s_bc, k = 1;
  if (s_ca < best) best = s_ca, k = 2;
  float u[3], v[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    u[d] = k == 0 ? a[d] : k == 1 ? b[d] : c[d];
    v[d] = k == 0 ? b[d] : k == 1 ? c[d] : a[d];
  }
  const float t = mr_seg_t(p, u, v);
#pragma unroll
  for (int d = 0; d < 3; ++d) x[d] = u[d] + t * (v[d] - u[d]);
  float ab[3], ac[3], n[3];
  mesh_sub(b, a, ab);
  mesh_sub(c, a, ac);
  mesh_cross(ab, ac, n);
  const float nn = mesh_dot(n, n);
  if (nn > 0.f) {
    float ap[3], bp[3], cp[3], bc[3], ca[3], w[3];
    mesh_sub(p, a, ap);
    mesh_sub(p, b, bp);
    mesh_sub(p, c, cp);
    mesh_sub(c, b, bc);
    mesh_sub(a, c, ca);
    mesh_cross(ab, ap, w);
    const float s0 = mesh_dot(n, w);
    mesh_cross(bc, bp, w);
    const float s1 = mesh_dot(n, w);
    mesh_cross(ca, cp, w);
    const float s2 = mesh_dot(n, w);
    if (s0 >= 0.f && s1 >= 0.f && s2 >= 0.f) {
      const float h = mesh_dot(n, ap);
      if ((h * h) / nn <= best) {
        const float g = h / nn;
#pragma unroll
        for (int d = 0; d < 3; ++d) x[d] = p[d] - g * n[d];
      }
    }
  }
  mr_unit(n, nn, nrm);
}

__global__ __launch_bounds__(MR_THREADS) void meshreg_closest_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                                     const int* __restrict__ faces, int64_t n_faces,
                                                                     const float* __restrict__ vnormals, const float* __restrict__ points,
                                                                     const int* __restrict__ face, int64_t n, float* __restrict__ x,
                                                                     float* __restrict__ nrm) {
  const int64_t i = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  float xo[3] = {p[0], p[1], p[2]}, no[3] = {0.f, 0.f, 0.f};
  const int64_t f = face[i];
  float a[3], b[3], c[3];
  if (f >= 0 && f < n_faces && mesh_finite(p[0]) && mesh_finite(p[1]) && mesh_finite(p[2]) && md_load(verts, n_verts, faces, f, a, b, c)) {
    mr_closest(p, a, b, c, xo, no);
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (vnormals && i0 == i1 && i1 == i2) {                 // a cloud's point: its own normal, normalised (0 if that fails)
      float v[3] = {vnormals[3 * (int64_t)i0], vnormals[3 * (int64_t)i0 + 1], vnormals[3 * (int64_t)i0 + 2]};
      const bool ok = mesh_normalise(v);
#pragma unroll
      for (int d = 0; d < 3; ++d) no[d] = ok ? v[d] : 0.f;
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    x[3 * i + d] = xo[d];
    nrm[3 * i + d] = no[d];
  }
}

__global__ __launch_bounds__(MR_THREADS) void meshreg_face_normals_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                                          const int* __restrict__ faces, int64_t n_faces,
                                                                          float* __restrict__ nrm) {
  const int64_t f = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (f >= n_faces) return;
  float a[3], b[3], c[3], no[3] = {0.f, 0.f, 0.f};
  if (md_load(verts, n_verts, faces, f, a, b, c)) {
    float ab[3], ac[3], n[3];
    mesh_sub(b, a, ab);
    mesh_sub(c, a, ac);
    mesh_cross(ab, ac, n);
    mr_unit(n, mesh_dot(n, n), no);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) nrm[3 * f + d] = no[d];
}

struct mr_centre {
  double c[3];
};

// one correspondence's 47 terms added to acc (the layout of include/mnerf.h)
__host__ __device__ __forceinline__ void mr_terms(const float* pf, const float* xf, const float* nf, const double* c, double* acc) {
  double p[3], x[3], n[3], pc[3], xc[3], d[3], J[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = (double)pf[k];
    x[k] = (double)xf[k];
    n[k] = (double)nf[k];
    pc[k] = p[k] - c[k];
    xc[k] = x[k] - c[k];
    d[k] = p[k] - x[k];
  }
  const double r = mesh_dot(d, n);
  mesh_cross(pc, n, J);
#pragma unroll
  for (int k = 0; k < 3; ++k) J[3 + k] = n[k];
  acc[0] += 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    acc[1 + k] += pc[k];
    acc[4 + k] += xc[k];
#pragma unroll
    for (int l = 0; l < 3; ++l) acc[7 + 3 * k + l] += pc[k] * xc[l];
  }
  acc[16] += mesh_dot(pc, pc);
  acc[17] += mesh_dot(xc, xc);
  acc[18] += mesh_dot(d, d);
  acc[19] += r * r;
  int at = 20;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int l = k; l < 6; ++l) acc[at++] += J[k] * J[l];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[41 + k] += J[k] * r;
}

__global__ __launch_bounds__(MR_THREADS) void meshreg_sums_kernel(const float* __restrict__ p, const float* __restrict__ x,
                                                                  const float* __restrict__ nrm, const uint8_t* __restrict__ keep, int64_t n,
                                                                  mr_centre centre, double* __restrict__ partials) {
  __shared__ double l_red[MR_ROUND][MR_THREADS];
  __shared__ double l_red2[MR_ROUND][16];
  const int t = threadIdx.x;
  double acc[MR_ACC];
#pragma unroll
  for (int k = 0; k < MR_ACC; ++k) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * MR_THREADS + t; i < n; i += (int64_t)gridDim.x * MR_THREADS) {
    if (keep[i] != 0) mr_terms(p + 3 * i, x + 3 * i, nrm + 3 * i, centre.c, acc);
  }
  // the workgroup's sums, 16 at a time: thread (j, s) adds entries s, 16 + s, ... of accumulator j, then one thread adds the 16
  double* part = partials + (int64_t)blockIdx.x * MR_SUMS;
#pragma unroll
  for (int round = 0; round < MR_ACC / MR_ROUND; ++round) {
#pragma unroll
    for (int j = 0; j < MR_ROUND; ++j) l_red[j][t] = acc[round * MR_ROUND + j];
    __syncthreads();
    {
      const int j = t >> 4, s = t & 15;
      double sum = 0.0;
      for (int k = 0; k < 16; ++k) sum += l_red[j][16 * k + s];
      l_red2[j][s] = sum;
    }
    __syncthreads();
    if (t < MR_ROUND && round * MR_ROUND + t < MR_SUMS) {
      double sum = 0.0;
      for (int k = 0; k < 16; ++k) sum += l_red2[t][k];
      part[round * MR_ROUND + t] = sum;
    }
    __syncthreads();
  }
}

// second stage: thread (q, e), q = 0 .. 3, adds the partials of entry e over the q-th quarter of the workgroups in ascending order,
// then thread e adds the four in order.  blocks == 0 (no correspondence at all): every entry is 0.
#define MR_FINAL_PARTS 4
__global__ __launch_bounds__(MR_THREADS) void meshreg_sums_final_kernel(const double* __restrict__ partials, int blocks, double* __restrict__ out) {
  __shared__ double l_part[MR_FINAL_PARTS][64];
  const int t = threadIdx.x, q = t >> 6, e = t & 63;
  if (e < MR_SUMS) {
    const int chunk = (blocks + MR_FINAL_PARTS - 1) / MR_FINAL_PARTS;
    const int b0 = q * chunk, b1 = min(b0 + chunk, blocks);
    double s = 0.0;
    for (int b = b0; b < b1; ++b) s += partials[(int64_t)b * MR_SUMS + e];
    l_part[q][e] = s;
  }
  __syncthreads();
  if (t < MR_SUMS) {
    double s = 0.0;
    for (int k = 0; k < MR_FINAL_PARTS; ++k) s += l_part[k][t];
    out[t] = s;
  }
}

__global__ __launch_bounds__(MR_THREADS) void meshreg_crop_kernel(const float* __restrict__ points, int64_t n, const double* __restrict__ polygon,
                                                                  int m, int iu, int iv, int iw, double w_min, double w_max,
                                                                  uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (i >= n) return;
  const double pu = (double)points[3 * i + iu], pv = (double)points[3 * i + iv], pw = (double)points[3 * i + iw];
  bool odd = false;
  double au = polygon[0], av = polygon[1];                  // edge (k, k + 1 mod m): P_i = (au, av), P_j = (bu, bv)
  for (int k = 0; k < m; ++k) {
    const int j = k + 1 < m ? k + 1 : 0;
    const double bu = polygon[2 * j], bv = polygon[2 * j + 1];
    if ((av > pv) != (bv > pv) && pu < ((bu - au) * (pv - av)) / (bv - av) + au) odd = !odd;
    au = bu;
    av = bv;
  }
  keep[i] = (w_min <= pw && pw <= w_max && odd) ? 1 : 0;
}

static int mr_blocks(int64_t n) {
  const int64_t b = (n + MR_THREADS - 1) / MR_THREADS;
  return (int)(b < MR_MAX_BLOCKS ? b : MR_MAX_BLOCKS);
}

extern "C" int mnr_mesh_closest(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, const float* vnormals,
                                const float* points, const int* face, int64_t n, float* x, float* nrm, void* stream) {
  const int st = md_check_mesh("mnr_mesh_closest", verts, n_verts, faces, n_faces);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG(n >= 0 && n < (1ll << 31), "mnr_mesh_closest: n = %lld must lie in 0 .. 2^31 - 1", (long long)n);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(points && face && x && nrm, "mnr_mesh_closest: needs points [n,3], face [n], x [n,3] and nrm [n,3]");
  hipLaunchKernelGGL(meshreg_closest_kernel, dim3((unsigned)mnr_cdiv(n, MR_THREADS)), dim3(MR_THREADS), 0, (hipStream_t)stream, verts, n_verts,
                     faces, n_faces, vnormals, points, face, n, x, nrm);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mesh_face_normals(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, float* nrm, void* stream) {
  const int st = md_check_mesh("mnr_mesh_face_normals", verts, n_verts, faces, n_faces);
  if (st != MNR_OK) return st;
  if (n_faces == 0) return MNR_OK;
  MNR_CHECK_ARG(nrm, "mnr_mesh_face_normals: needs nrm [n_faces,3]");
  hipLaunchKernelGGL(meshreg_face_normals_kernel, dim3((unsigned)mnr_cdiv(n_faces, MR_THREADS)), dim3(MR_THREADS), 0, (hipStream_t)stream, verts,
                     n_verts, faces, n_faces, nrm);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_icp_sums_partials(int64_t n) { return n > 0 && n < (1ll << 31) ? mr_blocks(n) * MR_SUMS : 0; }

extern "C" int mnr_icp_sums(int64_t n, const float* p, const float* x, const float* nrm, const uint8_t* keep, const double* centre,
                            double* partials, double* out, void* stream) {
  MNR_CHECK_ARG(n >= 0 && n < (1ll << 31), "mnr_icp_sums: n = %lld must lie in 0 .. 2^31 - 1", (long long)n);
  MNR_CHECK_ARG(out && centre, "mnr_icp_sums: needs centre [3] (host) and out [%d]", MR_SUMS);
  MNR_CHECK_ARG(mesh_finite(centre[0]) && mesh_finite(centre[1]) && mesh_finite(centre[2]), "mnr_icp_sums: the centre (%g, %g, %g) must be finite",
                centre[0], centre[1], centre[2]);
  MNR_CHECK_ARG(n == 0 || (p && x && nrm && keep && partials),
                "mnr_icp_sums: needs p, x, nrm [n,3], keep [n] and the partials workspace of mnr_icp_sums_partials(n) doubles");
  const int blocks = n > 0 ? mr_blocks(n) : 0;
  if (blocks > 0) {
    mr_centre c;
    for (int d = 0; d < 3; ++d) c.c[d] = centre[d];
    hipLaunchKernelGGL(meshreg_sums_kernel, dim3(blocks), dim3(MR_THREADS), 0, (hipStream_t)stream, p, x, nrm, keep, n, c, partials);
    MNR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(meshreg_sums_final_kernel, dim3(1), dim3(MR_THREADS), 0, (hipStream_t)stream, partials, blocks, out);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_crop_polygon(const float* points, int64_t n, const double* polygon, int m, int axis, double w_min, double w_max,
                                uint8_t* keep, void* stream) {
  MNR_CHECK_ARG(n >= 0 && n < (1ll << 31), "mnr_crop_polygon: n = %lld must lie in 0 .. 2^31 - 1", (long long)n);
  MNR_CHECK_ARG(m >= 3 && m <= MNR_CROP_MAX_POLYGON, "mnr_crop_polygon: a polygon of %d corners: must have 3 .. %d", m, MNR_CROP_MAX_POLYGON);
  MNR_CHECK_ARG(axis >= 0 && axis <= 2, "mnr_crop_polygon: axis = %d must be 0 (X), 1 (Y) or 2 (Z)", axis);
  MNR_CHECK_ARG(w_min <= w_max, "mnr_crop_polygon: needs w_min <= w_max, are %g and %g", w_min, w_max);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(points && polygon && keep, "mnr_crop_polygon: needs points [n,3], polygon [m,2] and keep [n]");
  const int iu = axis == 0 ? 1 : 0, iv = axis == 2 ? 1 : 2;
  hipLaunchKernelGGL(meshreg_crop_kernel, dim3((unsigned)mnr_cdiv(n, MR_THREADS)), dim3(MR_THREADS), 0, (hipStream_t)stream, points, n, polygon, m,
                     iu, iv, axis, w_min, w_max, keep);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
