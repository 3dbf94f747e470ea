// Mesh clean-up on device (gfx950): connected components of an indexed triangle mesh, and simplification by vertex clustering
// with quadric-error placement (Lindstrom 2000, DeCoro-Tatarchuk 2007).  include/mnerf.h states both contracts, the order of every
// sum included; tests/mesh_clean_ref.py restates them in NumPy.  Sorting, unique, scans and compaction are the caller's
// (multinerf_amd/mesh.py, torch on the device): these kernels are the per-element work between them.
//
// Components.  labels[v] converges to the smallest vertex id v is connected to.  Two invariants hold from mnr_mesh_cc_init on
// and under every interleaving: labels[v] <= v, and labels[v] is a vertex of v's component.  A sweep is two launches:
//   hook  one thread a face: m = min of the three labels; a vertex x whose label l is above m gets atomicMin(labels[x], m) and
//         its old representative atomicMin(labels[l], m) (so that a whole tree moves, not a vertex), and *changed = 1;
//   jump  one thread a vertex: follow l = labels[l] while it decreases, store the end (pointer jumping, racy reads of values that
//         only ever decrease to valid ones).
// A sweep whose hook launch changes nothing is the fixed point: every face then has one label, so a component has one label L,
// L is one of its vertices, and its smallest vertex m has labels[m] <= m inside the component, i.e. labels[m] = m = L.  The result
// is therefore unique however the atomics interleave: integer min, no floating point, two runs agree bit for bit.  The flag is a
// plain store of 1 (every writer stores the same value).  Every index read from faces or labels is checked against [0, V)
// before it is used as one: no access leaves labels whatever the inputs hold.
//
// Clustering.  keys: one thread a vertex.  solve: one thread a CLUSTER walks its member list and its face list in the stated
// order with its sums in registers (float64: 6 + 3 of the quadric, 3 + 3 of the centroid and normal, the 9 coordinates of the
// face in flight): no atomics, no reduction tree, the order of the sums is the order of the lists.  A cluster at a cell of 2
// grid spacings has about 4 members and 20 faces, so a wave a cluster would idle most lanes; a thread a cluster gathers
// float32 triples through the lists (uncoalesced, L2-resident: a mesh is a few tens of MB) and is bound by those gathers, not
// by the float64 arithmetic.  faces: one thread a face.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define MC_THREADS 256
#define MC_INF __builtin_huge_val()

static_assert(MNR_MESH_CELL_LIMIT == (1 << 21), "three cell indices of 21 bits fill a key");

// ---- connected components

__global__ __launch_bounds__(MC_THREADS) void mesh_cc_init_kernel(int* __restrict__ labels, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (v < V) labels[v] = (int)v;
}

__global__ __launch_bounds__(MC_THREADS) void mesh_cc_hook_kernel(const int* __restrict__ faces, int64_t T, int64_t V, int* labels,
                                                                  int* changed) {
  const int64_t f = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (f >= T) return;
  int x[3], l[3];
  if (!mesh_face_ids(faces, f, V, x)) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    l[s] = labels[x[s]];
    if (l[s] < 0 || l[s] >= V) return;
  }
  const int m = min(l[0], min(l[1], l[2]));
  bool moved = false;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (l[s] > m) {
      atomicMin(&labels[l[s]], m);
      atomicMin(&labels[x[s]], m);
      moved = true;
    }
  }
  if (moved) *changed = 1;
}

__global__ __launch_bounds__(MC_THREADS) void mesh_cc_jump_kernel(int* labels, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (v >= V) return;
  int l = labels[v];
  if (l < 0 || l >= V) return;
  for (;;) {
    const int n = labels[l];
    if (n < 0 || n >= l) break;                             // a root (n == l); n > l cannot happen after mnr_mesh_cc_init
    l = n;
  }
  labels[v] = l;
}

extern "C" int mnr_mesh_cc_init(int64_t n_verts, int* labels, void* stream) {
  MNR_CHECK_ARG(n_verts >= 0 && n_verts < (1ll << 31), "mnr_mesh_cc_init: %lld vertices, must lie in 0 .. 2^31 - 1", (long long)n_verts);
  if (n_verts == 0) return MNR_OK;
  MNR_CHECK_ARG(labels, "mnr_mesh_cc_init: needs labels [n_verts]");
  hipLaunchKernelGGL(mesh_cc_init_kernel, dim3((unsigned)mnr_cdiv(n_verts, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, labels,
                     n_verts);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

extern "C" int mnr_mesh_cc_sweep(const int* faces, int64_t n_faces, int64_t n_verts, int* labels, int* changed, void* stream) {
  MNR_CHECK_ARG(n_verts >= 0 && n_verts < (1ll << 31), "mnr_mesh_cc_sweep: %lld vertices, must lie in 0 .. 2^31 - 1", (long long)n_verts);
  MNR_CHECK_ARG(n_faces >= 0 && n_faces < (1ll << 31), "mnr_mesh_cc_sweep: %lld faces, must lie in 0 .. 2^31 - 1", (long long)n_faces);
  if (n_verts == 0 || n_faces == 0) return MNR_OK;
  MNR_CHECK_ARG(faces && labels && changed, "mnr_mesh_cc_sweep: needs faces [n_faces,3], labels [n_verts] and the changed flag");
  hipLaunchKernelGGL(mesh_cc_hook_kernel, dim3((unsigned)mnr_cdiv(n_faces, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, faces,
                     n_faces, n_verts, labels, changed);
  MNR_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_cc_jump_kernel, dim3((unsigned)mnr_cdiv(n_verts, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, labels,
                     n_verts);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---- vertex clustering: keys

struct mc_grid {
  float o[3];
  float cell;
};

__global__ __launch_bounds__(MC_THREADS) void mesh_cluster_keys_kernel(const float* __restrict__ verts, int64_t V, mc_grid g,
                                                                       int64_t* __restrict__ keys) {
  const int64_t v = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (v >= V) return;
  int64_t key = 0;
  bool finite = true, inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = verts[3 * v + a];
    finite = finite && mesh_finite(x);
    const float q = floorf((x - g.o[a]) / g.cell);
    const bool ok = q >= 0.f && q < (float)MNR_MESH_CELL_LIMIT;
    inside = inside && ok;
    key = (key << 21) | (int64_t)(ok ? (int)q : 0);
  }
  keys[v] = !finite ? MNR_MESH_KEY_NONFINITE : !inside ? MNR_MESH_KEY_OUTSIDE : key;
}

static int mc_check_grid(const char* name, const float* origin, float cell) {
  MNR_CHECK_ARG(origin, "%s: needs origin [3] (host)", name);
  for (int d = 0; d < 3; ++d) MNR_CHECK_ARG(mesh_finite(origin[d]), "%s: the origin must be finite", name);
  MNR_CHECK_ARG(cell > 0.f && cell <= MNR_F32_MAX, "%s: cell must be positive and finite, is %g", name, (double)cell);
  return MNR_OK;
}

extern "C" int mnr_mesh_cluster_keys(const float* verts, int64_t n_verts, const float* origin, float cell, int64_t* keys, void* stream) {
  MNR_CHECK_ARG(n_verts >= 0 && n_verts < (1ll << 31), "mnr_mesh_cluster_keys: %lld vertices, must lie in 0 .. 2^31 - 1", (long long)n_verts);
  const int st = mc_check_grid("mnr_mesh_cluster_keys", origin, cell);
  if (st != MNR_OK) return st;
  if (n_verts == 0) return MNR_OK;
  MNR_CHECK_ARG(verts && keys, "mnr_mesh_cluster_keys: needs verts [n_verts,3] and keys [n_verts]");
  mc_grid g;
  for (int d = 0; d < 3; ++d) g.o[d] = origin[d];
  g.cell = cell;
  hipLaunchKernelGGL(mesh_cluster_keys_kernel, dim3((unsigned)mnr_cdiv(n_verts, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, verts,
                     n_verts, g, keys);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---- vertex clustering: per-cluster accumulate, solve, attributes

template <bool COLOR>
__global__ __launch_bounds__(MC_THREADS) void mesh_cluster_solve_kernel(mnr_mesh_cluster_args a) {
  const int64_t k = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (k >= a.n_clusters) return;
  const int64_t key = a.keys[k];
  const double cell = (double)a.cell;
  double m[3];                                              // the cell's centre
  m[0] = (double)a.origin[0] + cell * ((double)((key >> 42) & 0x1fffff) + 0.5);
  m[1] = (double)a.origin[1] + cell * ((double)((key >> 21) & 0x1fffff) + 0.5);
  m[2] = (double)a.origin[2] + cell * ((double)(key & 0x1fffff) + 0.5);

  // members, ascending id: centroid, normal, colour
  int64_t v0 = a.member_start[k], v1 = a.member_start[k + 1];
  v0 = v0 < 0 ? 0 : v0;
  v1 = v1 > a.n_verts ? a.n_verts : v1;
  double sg[3] = {0., 0., 0.}, sn[3] = {0., 0., 0.};
  unsigned long long sc[3] = {0ull, 0ull, 0ull}, count = 0ull;
  for (int64_t n = v0; n < v1; ++n) {
    const int v = a.members[n];
    if (v < 0 || v >= a.n_verts) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sg[c] += (double)a.verts[3 * (int64_t)v + c] - m[c];
      sn[c] += (double)a.normals[3 * (int64_t)v + c];
      if (COLOR) sc[c] += a.colors[3 * (int64_t)v + c];
    }
    ++count;
  }
  double g[3] = {0., 0., 0.};
  if (count > 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = sg[c] / (double)count;
  }

  // faces, ascending id: the area-weighted quadric  A = sum n n^T / L,  r = sum n (n . a) / L
  int64_t f0 = a.face_start[k], f1 = a.face_start[k + 1];
  f0 = f0 < 0 ? 0 : f0;
  f1 = f1 > a.n_incident ? a.n_incident : f1;
  double A00 = 0., A01 = 0., A02 = 0., A11 = 0., A12 = 0., A22 = 0., r0 = 0., r1 = 0., r2 = 0.;
  for (int64_t n = f0; n < f1; ++n) {
    const int f = a.cluster_faces[n];
    if (f < 0 || f >= a.n_faces) continue;
    const int ia = a.faces[3 * (int64_t)f], ib = a.faces[3 * (int64_t)f + 1], ic = a.faces[3 * (int64_t)f + 2];
    if (ia < 0 || ia >= a.n_verts || ib < 0 || ib >= a.n_verts || ic < 0 || ic >= a.n_verts) continue;      // (mesh_face_ids gives other device code here)
    double pa[3], e1[3], e2[3], nf[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pa[c] = (double)a.verts[3 * (int64_t)ia + c] - m[c];
      const double pb = (double)a.verts[3 * (int64_t)ib + c] - m[c], pc = (double)a.verts[3 * (int64_t)ic + c] - m[c];
      e1[c] = pb - pa[c];
      e2[c] = pc - pa[c];
    }
    mesh_cross(e1, e2, nf);
    const double n0 = nf[0], n1 = nf[1], n2 = nf[2];
    const double L = sqrt(mesh_dot(nf, nf));
    if (!(L > 0. && L < MC_INF)) continue;
    const double d = mesh_dot(nf, pa);
    A00 += (n0 * n0) / L;
    A01 += (n0 * n1) / L;
    A02 += (n0 * n2) / L;
    A11 += (n1 * n1) / L;
    A12 += (n1 * n2) / L;
    A22 += (n2 * n2) / L;
    r0 += (n0 * d) / L;
    r1 += (n1 * d) / L;
    r2 += (n2 * d) / L;
  }

  // (A + lam I) x = r + lam g by cofactors
  const double tr = (A00 + A11) + A22;
  const double lam = (MNR_QEM_REG * tr) / 3.0;
  const double M00 = A00 + lam, M11 = A11 + lam, M22 = A22 + lam;
  const double b0 = r0 + lam * g[0], b1 = r1 + lam * g[1], b2 = r2 + lam * g[2];
  const double c00 = M11 * M22 - A12 * A12, c01 = A02 * A12 - A01 * M22, c02 = A01 * A12 - A02 * M11;
  const double c11 = M00 * M22 - A02 * A02, c12 = A01 * A02 - M00 * A12, c22 = M00 * M11 - A01 * A01;
  const double det = (M00 * c00 + A01 * c01) + A02 * c02;
  double x[3];
  x[0] = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
  x[1] = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
  x[2] = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
  const double half = cell / 2.0;
  const bool take = tr > 0. && mesh_finite(x[0]) && mesh_finite(x[1]) && mesh_finite(x[2]) && fabs(x[0]) <= half && fabs(x[1]) <= half &&
                    fabs(x[2]) <= half;
  const double len = sqrt(mesh_dot(sn, sn));
  const bool unit = len > 0. && len < MC_INF;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.out_verts[3 * k + c] = (float)(m[c] + (take ? x[c] : g[c]));
    a.out_normals[3 * k + c] = unit ? (float)(sn[c] / len) : 0.f;
    if (COLOR) a.out_colors[3 * k + c] = count > 0 ? (unsigned char)((2ull * sc[c] + count) / (2ull * count)) : (unsigned char)0;
  }
  if (a.fallback != nullptr) a.fallback[k] = take ? 0 : 1;
}

extern "C" int mnr_mesh_cluster_solve(const mnr_mesh_cluster_args* a, void* stream) {
  MNR_CHECK_ARG(a, "mnr_mesh_cluster_solve: needs its arguments");
  MNR_CHECK_ARG(a->n_verts >= 0 && a->n_verts < (1ll << 31) && a->n_faces >= 0 && a->n_faces < (1ll << 31),
                "mnr_mesh_cluster_solve: %lld vertices and %lld faces, both must lie in 0 .. 2^31 - 1", (long long)a->n_verts, (long long)a->n_faces);
  MNR_CHECK_ARG(a->n_clusters >= 0 && a->n_clusters <= a->n_verts, "mnr_mesh_cluster_solve: %lld clusters of %lld vertices",
                (long long)a->n_clusters, (long long)a->n_verts);
  MNR_CHECK_ARG(a->n_incident >= 0 && a->n_incident <= 3 * a->n_faces, "mnr_mesh_cluster_solve: %lld face list entries for %lld faces",
                (long long)a->n_incident, (long long)a->n_faces);
  const int st = mc_check_grid("mnr_mesh_cluster_solve", a->origin, a->cell);
  if (st != MNR_OK) return st;
  MNR_CHECK_ARG((a->colors != nullptr) == (a->out_colors != nullptr), "mnr_mesh_cluster_solve: colors and out_colors are both given or both NULL");
  if (a->n_clusters == 0) return MNR_OK;
  MNR_CHECK_ARG(a->verts && a->normals && a->keys && a->member_start && a->members && a->face_start,
                "mnr_mesh_cluster_solve: needs verts, normals, keys, member_start, members and face_start");
  MNR_CHECK_ARG(a->n_incident == 0 || (a->faces && a->cluster_faces), "mnr_mesh_cluster_solve: needs faces and cluster_faces");
  MNR_CHECK_ARG(a->out_verts && a->out_normals, "mnr_mesh_cluster_solve: needs out_verts and out_normals [n_clusters,3]");
  const dim3 grid((unsigned)mnr_cdiv(a->n_clusters, MC_THREADS)), block(MC_THREADS);
  if (a->colors != nullptr) hipLaunchKernelGGL(mesh_cluster_solve_kernel<true>, grid, block, 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(mesh_cluster_solve_kernel<false>, grid, block, 0, (hipStream_t)stream, *a);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---- vertex clustering: per-face re-index, classify, canonical rotation

__global__ __launch_bounds__(MC_THREADS) void mesh_cluster_faces_kernel(const int* __restrict__ faces, int64_t T, const int* __restrict__ map,
                                                                        int64_t V, int64_t K, int* __restrict__ mapped, int* __restrict__ canon,
                                                                        int* __restrict__ incident, unsigned char* __restrict__ keep) {
  const int64_t f = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (f >= T) return;
  int c[3];
  bool ok = true;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int x = faces[3 * f + s];
    c[s] = -1;
    if (x >= 0 && x < V) c[s] = map[x];
    ok = ok && c[s] >= 0 && c[s] < K;
  }
  if (!ok) {                                                // an index outside the mesh: the face belongs to no cluster and is dropped
#pragma unroll
    for (int s = 0; s < 3; ++s) mapped[3 * f + s] = canon[3 * f + s] = incident[3 * f + s] = -1;
    keep[f] = 0;
    return;
  }
  const int r = (c[0] <= c[1] && c[0] <= c[2]) ? 0 : (c[1] <= c[2] ? 1 : 2);        // the smallest cluster comes first
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    mapped[3 * f + s] = c[s];
    canon[3 * f + s] = c[(r + s) % 3];
  }
  incident[3 * f] = c[0];
  incident[3 * f + 1] = c[1] != c[0] ? c[1] : -1;
  incident[3 * f + 2] = (c[2] != c[0] && c[2] != c[1]) ? c[2] : -1;
  keep[f] = (c[0] != c[1] && c[1] != c[2] && c[0] != c[2]) ? 1 : 0;
}

extern "C" int mnr_mesh_cluster_faces(const int* faces, int64_t n_faces, const int* map, int64_t n_verts, int64_t n_clusters, int* mapped,
                                      int* canon, int* incident, unsigned char* keep, void* stream) {
  MNR_CHECK_ARG(n_verts >= 0 && n_verts < (1ll << 31) && n_faces >= 0 && n_faces < (1ll << 31),
                "mnr_mesh_cluster_faces: %lld vertices and %lld faces, both must lie in 0 .. 2^31 - 1", (long long)n_verts, (long long)n_faces);
  MNR_CHECK_ARG(n_clusters >= 0 && n_clusters <= n_verts, "mnr_mesh_cluster_faces: %lld clusters of %lld vertices", (long long)n_clusters,
                (long long)n_verts);
  if (n_faces == 0) return MNR_OK;
  MNR_CHECK_ARG(faces && (map || n_verts == 0), "mnr_mesh_cluster_faces: needs faces [n_faces,3] and map [n_verts]");
  MNR_CHECK_ARG(mapped && canon && incident && keep, "mnr_mesh_cluster_faces: needs mapped, canon, incident [n_faces,3] and keep [n_faces]");
  hipLaunchKernelGGL(mesh_cluster_faces_kernel, dim3((unsigned)mnr_cdiv(n_faces, MC_THREADS)), dim3(MC_THREADS), 0, (hipStream_t)stream, faces,
                     n_faces, map, n_verts, n_clusters, mapped, canon, incident, keep);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
