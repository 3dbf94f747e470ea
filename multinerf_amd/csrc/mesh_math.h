// The arithmetic and the index check that the six mesh files share (mesh.hip, tsdf.hip, meshclean.hip, atlas.hip, raster.hip,
// meshdist.hip).  Each of them promises every floating-point operation in a stated order, bit for bit against a NumPy
// restatement, so each helper fixes its order once, for all of them.
#pragma once

#include "common.h"

// The pragma is HERE, not left to the includer: a file that includes this header in front of its own pragma would otherwise
// compile these bodies with contraction on, and the kernels that inline them would fuse multiplies and adds and silently drift
// from their restatements.  It stays in force for the rest of the including file; all six switch contraction off anyway.
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
