// The arithmetic and the index check that the seven mesh files share (mesh.hip, tsdf.hip, meshclean.hip, atlas.hip, raster.hip,
// meshdist.hip, meshreg.hip).  Each of them promises every floating-point operation in a stated order, bit for bit against a NumPy
// restatement, so each helper fixes its order once, for all of them.
#pragma once

#include "common.h"

// The pragma is HERE, not left to the includer: a file that includes this header in front of its own pragma would otherwise
// compile these bodies with contraction on, and the kernels that inline them would fuse multiplies and adds and silently drift
// from their restatements.  It stays in force for the rest of the including file; all seven switch contraction off anyway.
#pragma clang fp contract(off)

__host__ __device__ __forceinline__ bool mesh_finite(float x) { return x - x == 0.f; }
__host__ __device__ __forceinline__ bool mesh_finite(double x) { return x - x == 0.0; }

template <typename T>
__host__ __device__ __forceinline__ T mesh_dot(const T* x, const T* y) {
  return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

template <typename T>
__host__ __device__ __forceinline__ void mesh_cross(const T* u, const T* v, T* o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}

template <typename T>
__host__ __device__ __forceinline__ void mesh_sub(const T* x, const T* y, T* o) {
  o[0] = x[0] - y[0];
  o[1] = x[1] - y[1];
  o[2] = x[2] - y[2];
}

// n / |n| in place; false (n untouched): the length is 0 or not finite
__host__ __device__ __forceinline__ bool mesh_normalise(float* n) {
  const float len = sqrtf(mesh_dot(n, n));
  if (!(len > 0.f && len <= MNR_F32_MAX)) return false;
  n[0] = n[0] / len;
  n[1] = n[1] / len;
  n[2] = n[2] / len;
  return true;
}

// the three vertex indices of face f; false: one lies outside [0, n_verts) and must not be used as an index
__host__ __device__ __forceinline__ bool mesh_face_ids(const int* __restrict__ faces, int64_t f, int64_t n_verts, int* id) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    id[k] = faces[3 * f + k];
    if (id[k] < 0 || id[k] >= n_verts) return false;
  }
  return true;
}

// ---- the point-to-face distance of include/mnerf.h ("Mesh geometry"), shared by meshdist.hip and meshreg.hip

__host__ __device__ __forceinline__ float md_seg(const float* p, const float* u, const float* v) {
  float uv[3], up[3], e[3];
  mesh_sub(v, u, uv);
  mesh_sub(p, u, up);
  const float L = mesh_dot(uv, uv);
  float t = 0.f;
  if (L > 0.f) t = fminf(fmaxf(mesh_dot(up, uv) / L, 0.f), 1.f);
#pragma unroll
  for (int d = 0; d < 3; ++d) e[d] = up[d] - t * uv[d];
  return mesh_dot(e, e);
}

// the squared distance of include/mnerf.h
__host__ __device__ __forceinline__ float md_d2(const float* p, const float* a, const float* b, const float* c) {
  float d2 = fminf(fminf(md_seg(p, a, b), md_seg(p, b, c)), md_seg(p, c, a));
  float ab[3], ac[3], n[3];
  mesh_sub(b, a, ab);
  mesh_sub(c, a, ac);
  mesh_cross(ab, ac, n);
  const float nn = mesh_dot(n, n);
  if (nn > 0.f) {
    float ap[3], bp[3], cp[3], bc[3], ca[3], x[3];
    mesh_sub(p, a, ap);
    mesh_sub(p, b, bp);
    mesh_sub(p, c, cp);
    mesh_sub(c, b, bc);
    mesh_sub(a, c, ca);
    mesh_cross(ab, ap, x);
    const float s0 = mesh_dot(n, x);
    mesh_cross(bc, bp, x);
    const float s1 = mesh_dot(n, x);
    mesh_cross(ca, cp, x);
    const float s2 = mesh_dot(n, x);
    if (s0 >= 0.f && s1 >= 0.f && s2 >= 0.f) {
      const float h = mesh_dot(n, ap);
      d2 = fminf(d2, (h * h) / nn);
    }
  }
  return d2;
}

// the corners of face f; false: the face is not valid (an index outside the vertices, a coordinate that is not finite)
__device__ __forceinline__ bool md_load(const float* __restrict__ verts, int64_t n_verts, const int* __restrict__ faces, int64_t f, float* a,
                                        float* b, float* c) {
  int id[3];
  if (!mesh_face_ids(faces, f, n_verts, id)) return false;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a[d] = verts[3 * (int64_t)id[0] + d];
    b[d] = verts[3 * (int64_t)id[1] + d];
    c[d] = verts[3 * (int64_t)id[2] + d];
    ok = ok && mesh_finite(a[d]) && mesh_finite(b[d]) && mesh_finite(c[d]);
  }
  return ok;
}

// the argument check of every entry point that takes a mesh (host)
static inline int md_check_mesh(const char* name, const float* verts, int64_t n_verts, const int* faces, int64_t n_faces) {
  MNR_CHECK_ARG(n_verts >= 0 && n_verts < (1ll << 31) && n_faces >= 0 && n_faces < (1ll << 31) - 1,
                "%s: %lld vertices and %lld faces: vertices must lie in 0 .. 2^31 - 1, faces in 0 .. 2^31 - 2", name, (long long)n_verts,
                (long long)n_faces);
  MNR_CHECK_ARG(n_faces == 0 || (faces && (n_verts == 0 || verts)), "%s: needs verts [n_verts,3] and faces [n_faces,3]", name);
  return MNR_OK;
}
