// TSDF fusion of depth images into a regular grid (Curless-Levoy / KinectFusion), and the validity of marching-tetrahedra
// vertices against a mask of observed voxels, on device (gfx950).
//
// Grid.  csrc/mesh.hip's: voxel (i, j, k) at origin + spacing (i, j, k), linear index p = (i ny + j) nz + k (64-bit).
//
// mnr_tsdf_integrate.  Per voxel, frames f = 0 .. F - 1 in ascending order (include/mnerf.h states the seven steps): project
// with the frame's [3,4] matrix, take the NEAREST pixel (pixel px covers [px, px + 1)), and add one observation t in [-1, 1]
// of weight 1: t = 1 where the ray is empty (acc below the threshold), min(1, (depth - zc) / trunc) where the voxel is in front
// of the surface or within the truncation behind it, nothing where it is occluded beyond the truncation.  The sums of the call
// are folded into the running averages once, after the last frame: a call reads and writes each volume once whatever F is.
// No atomics: a voxel belongs to one thread, two runs agree bit for bit.
//
// Arithmetic: float32 in the order written (contraction off), so that a NumPy float32 restatement (tests/tsdf_ref.py)
// reproduces the volumes bit for bit.
//
// Mapping.  The work is points x F projections and depth gathers.  A workgroup of 256 threads owns a BRICK of 4 x 8 x 8 voxels
// (k fastest: thread t holds (t >> 6, (t >> 3) & 7, t & 7), one wave one 8 x 8 slab), so that a wave's gathers fall on a few
// neighbouring image rows instead of along a 256-voxel line, and its volume accesses are 8 runs of 32 bytes.  Bricks at the far
// faces are ragged.  The F matrices are staged in LDS once per workgroup (TSDF_MAX_FRAMES = 64 of them, 3 KiB: the host entry
// loops over longer stacks, 64 frames a launch, and each launch then folds its own sums).
//
// Culling.  Before the per-voxel loop, wave 0 takes one frame a lane and projects the brick's 8 corners; a frame is dropped when
// every voxel of the brick would skip it in step 2 or 3, and the survivors are compacted in ascending order into an LDS list
// (one __ballot).  m_r is linear in the position and the voxels' float coordinates lie in the box of the corners' (float
// multiplication and addition are monotone), so in exact arithmetic "m_r < 0 at the 8 corners" carries over to every voxel; in
// float32 each m_r is off by at most 4 roundings, |fl(m_r) - m_r| <= 2.4e-7 mag_r with mag_r = |P_r0| max|x| + |P_r1| max|y| +
// |P_r2| max|z| + |P_r3|.  Hence the margins: a side is dropped only when the corners' float values clear it by
// 1e-6 mag_r (> 2 x 2.4e-7), and for the far sides (u >= W  <=>  m_0 - W zc >= 0 for zc > 0, the division being monotone and W a
// float) by 1e-6 (mag_0 + W mag_2), which also covers the two roundings of the test itself.  A NaN or an infinity anywhere
// makes the comparisons false: the frame is kept.  Culling therefore changes no result, only which frames are looked at.
//
// A plain mapping (256 consecutive linear indices a workgroup, no culling, the same per-voxel code) was measured against this
// one in the same session and was 2.9 to 5.8 times slower at 256^3 and 512^3 (profiles/tsdf_mesh.md); it is not kept.
//
// mnr_tsdf_integrate_cam.  The same fusion for a camera that has no [3,4] matrix (lens distortion, fisheye, the spherical 'pano'
// camera): steps 2 and 3 are cam_project (camera_project.h) on the frame's 28-float record, and the depth image holds s, the
// distance rendered along the camera's own rays, so step 5 compares d - s.  The brick mapping, the LDS staging (64 records,
// 7 KiB), one voxel a thread, ascending frames, the fold after the last frame and the 64-frames-a-launch loop are the ones
// above.  The kernel is templated on the model: a launch holds one model and no voxel branches on it.  mnr_tsdf_integrate and
// its kernel are not touched.
//
// Its culling.  Again it only decides which frames a brick looks at; each test implies that EVERY voxel of the brick would skip
// the frame in cam_project or in the on-image test, with margins that cover the float32 rounding on both sides.
//   Behind the camera (perspective only).  c_2 is linear in the position, so the 8-corner argument above carries over word for
//   word: the frame is dropped when c_2 < -1e-6 mag_2 at the 8 corners.  (u and v are NOT linear any more: no side tests.)
//   Field of view (perspective and fisheye).  The guard keeps a voxel only if its angle to the optical axis is at most alpha_max =
//   atan(sqrt(r2_max)) (perspective: X X + Y Y = tan^2) or sqrt(r2_max) (fisheye: theta itself).  The brick lies in the ball around
//   its centre m with radius rho = half its diagonal, and M is a rigid motion, so in the camera frame every voxel's angle is at
//   least A - beta, A = atan2(|(cm_0, cm_1)|, cm_2) the centre's angle and beta = asin(rho / |cm|), provided |cm| > rho.  The frame
//   is dropped when |cm| > rho' and A - beta' > alpha_max + 1e-3 with rho' = 1.01 rho + 1e-5 mag and beta' = asin(rho' / |cm|):
//   the inflation of rho by 1 % (and by the rounding of cm, <= 2.4e-7 mag a row) dwarfs the relative 1e-7 of the quotient, so
//   beta' >= beta in spite of asin's steepness near 1; atan2f, asinf, atanf and sqrtf are each within a few ulp of values <= pi,
//   i.e. 1e-6, and a voxel that the margin of 1e-3 rad lets through is looked at and decides for itself.  Conversely a voxel
//   beyond alpha_max + 1e-3 fails its own float32 guard: tan^2 (or theta^2) then exceeds r2_max by a relative 2e-3 / (sin cos)
//   (or 2e-3 / theta) at least, against 1e-6 of rounding in X X + Y Y.  An M that is not a rigid motion is refused on the host
//   (mesh.camera_record wants R^T R = 1 to 1e-4, covered by the 1 % of rho).
//   Pano sees every direction: nothing is culled.
// A NaN or an infinity anywhere makes the comparisons false: the frame is kept.
//
// mnr_mt_vertex_valid.  keep[id] = both ends of vertex id's grid edge are valid, from mesh.hip's mask / base: the id of edge
// (p, e) is base[p] + popcount(mask[p] & ((1 << e) - 1)).  ops.marching_tetrahedra(valid=...) compacts with it.
#include "mesh_math.h"                                      // (brings common.h)

#pragma clang fp contract(off)

#define TSDF_THREADS 256
#define TSDF_BI 4
#define TSDF_BJ 8
#define TSDF_BK 8
#define TSDF_INF __builtin_huge_valf()

static_assert(TSDF_BI * TSDF_BJ * TSDF_BK == TSDF_THREADS, "one voxel a thread");
static_assert(MNR_TSDF_MAX_FRAMES == 64, "the survivors' list is compacted with one 64-lane ballot");

// m_r = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3]
__device__ __forceinline__ float tsdf_row(const float* P, int r, float x, float y, float z) {
  return ((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3];
}

// true when every voxel of the brick with the corner coordinates cx / cy / cz [2] skips the frame of matrix P in step 2 or 3
__device__ __forceinline__ bool tsdf_brick_misses(const float* P, const float* cx, const float* cy, const float* cz, float Wf, float Hf) {
  const float ax = fmaxf(fabsf(cx[0]), fabsf(cx[1])), ay = fmaxf(fabsf(cy[0]), fabsf(cy[1])), az = fmaxf(fabsf(cz[0]), fabsf(cz[1]));
  float mag[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) mag[r] = ((fabsf(P[4 * r]) * ax + fabsf(P[4 * r + 1]) * ay) + fabsf(P[4 * r + 2]) * az) + fabsf(P[4 * r + 3]);
  const float tol0 = 1e-6f * mag[0], tol1 = 1e-6f * mag[1], tol2 = 1e-6f * mag[2];
  const float tolw = 1e-6f * (mag[0] + Wf * mag[2]), tolh = 1e-6f * (mag[1] + Hf * mag[2]);
  bool behind = true, left = true, right = true, top = true, bottom = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float x = cx[c & 1], y = cy[(c >> 1) & 1], z = cz[(c >> 2) & 1];
    const float m0 = tsdf_row(P, 0, x, y, z), m1 = tsdf_row(P, 1, x, y, z), m2 = tsdf_row(P, 2, x, y, z);
    behind = behind && m2 < -tol2;
    left = left && m0 < -tol0;
    top = top && m1 < -tol1;
    right = right && m0 - Wf * m2 > tolw;
    bottom = bottom && m1 - Hf * m2 > tolh;
  }
  return behind || left || right || top || bottom;
}

template <bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(mnr_tsdf_args a, int nbj, int nbk) {
  __shared__ float l_P[MNR_TSDF_MAX_FRAMES * 12];
  __shared__ int l_list[MNR_TSDF_MAX_FRAMES];
  __shared__ int l_count;
  const int t = threadIdx.x;
  for (int n = t; n < a.F * 12; n += TSDF_THREADS) l_P[n] = a.proj[n];

  const unsigned b = blockIdx.x, bij = b / (unsigned)nbk;
  const int bk = (int)(b - bij * (unsigned)nbk), bi = (int)(bij / (unsigned)nbj), bj = (int)(bij - (unsigned)bi * (unsigned)nbj);
  const int i = bi * TSDF_BI + (t >> 6), j = bj * TSDF_BJ + ((t >> 3) & 7), k = bk * TSDF_BK + (t & 7);
  __syncthreads();

  const float Wf = (float)a.W, Hf = (float)a.H;
  if (t < 64) {                                             // wave 0, one frame a lane
    bool keep = false;
    if (t < a.F) {
      const int ie = bi * TSDF_BI + TSDF_BI - 1, je = bj * TSDF_BJ + TSDF_BJ - 1, ke = bk * TSDF_BK + TSDF_BK - 1;
      const int i1 = ie < a.nx ? ie : a.nx - 1, j1 = je < a.ny ? je : a.ny - 1, k1 = ke < a.nz ? ke : a.nz - 1;
      const float cx[2] = {a.origin[0] + a.spacing * (float)(bi * TSDF_BI), a.origin[0] + a.spacing * (float)i1};
      const float cy[2] = {a.origin[1] + a.spacing * (float)(bj * TSDF_BJ), a.origin[1] + a.spacing * (float)j1};
      const float cz[2] = {a.origin[2] + a.spacing * (float)(bk * TSDF_BK), a.origin[2] + a.spacing * (float)k1};
      keep = !tsdf_brick_misses(l_P + 12 * t, cx, cy, cz, Wf, Hf);
    }
    const unsigned long long bal = __ballot(keep);
    if (keep) l_list[__popcll(bal & ((1ull << t) - 1ull))] = t;
    if (t == 0) l_count = __popcll(bal);
  }
  __syncthreads();
  const int count = l_count;
  if (!(i < a.nx && j < a.ny && k < a.nz)) return;

  const float x = a.origin[0] + a.spacing * (float)i, y = a.origin[1] + a.spacing * (float)j, z = a.origin[2] + a.spacing * (float)k;
  const size_t image = (size_t)a.H * (size_t)a.W;
  float sum_t = 0.f, sum_w = 0.f, sum_c[3] = {0.f, 0.f, 0.f};
  for (int n = 0; n < count; ++n) {
    const int f = l_list[n];
    const float* P = l_P + 12 * f;
    const float m0 = tsdf_row(P, 0, x, y, z), m1 = tsdf_row(P, 1, x, y, z), zc = tsdf_row(P, 2, x, y, z);
    if (!(zc > 0.f)) continue;
    const float u = m0 / zc, v = m1 / zc;
    if (!(u >= 0.f && u < Wf && v >= 0.f && v < Hf)) continue;
    const size_t pix = (size_t)f * image + (size_t)(int)v * (size_t)a.W + (size_t)(int)u;
    float obs;
    if (a.acc != nullptr && a.acc[pix] < a.acc_threshold) {
      obs = 1.f;
    } else {
      const float d = a.depth[pix];
      if (!(d > 0.f && d < TSDF_INF)) continue;
      const float s = d - zc;
      if (s < -a.trunc) continue;
      obs = s / a.trunc;
      obs = obs < 1.f ? obs : 1.f;
    }
    sum_t += obs;
    sum_w += 1.f;
    if (COLOR) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sum_c[c] += a.rgb[pix * 3 + c];
    }
  }
  if (!(sum_w > 0.f)) return;
  const int64_t p = ((int64_t)i * a.ny + j) * a.nz + k;
  const float W0 = a.weight[p], Wn = W0 + sum_w;
  a.tsdf[p] = (W0 * a.tsdf[p] + sum_t) / Wn;
  if (COLOR) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.color[p * 3 + c] = (W0 * a.color[p * 3 + c] + sum_c[c]) / Wn;
  }
  a.weight[p] = Wn;
}

extern "C" int mnr_tsdf_integrate(const mnr_tsdf_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->tsdf && a->weight, "mnr_tsdf_integrate: needs the tsdf and weight volumes");
  MNR_CHECK_ARG(a->nx >= 1 && a->ny >= 1 && a->nz >= 1, "mnr_tsdf_integrate: every grid dimension must be at least 1, got [%d, %d, %d]",
                a->nx, a->ny, a->nz);
  MNR_CHECK_ARG(a->spacing > 0.f && a->spacing <= MNR_F32_MAX, "mnr_tsdf_integrate: the spacing must be positive and finite, is %g",
                (double)a->spacing);
  MNR_CHECK_ARG(a->trunc > 0.f && a->trunc <= MNR_F32_MAX, "mnr_tsdf_integrate: trunc must be positive and finite, is %g", (double)a->trunc);
  for (int d = 0; d < 3; ++d) MNR_CHECK_ARG(mesh_finite(a->origin[d]), "mnr_tsdf_integrate: the origin must be finite");
  MNR_CHECK_ARG(a->F >= 0, "mnr_tsdf_integrate: F = %d frames", a->F);
  MNR_CHECK_ARG(a->H >= 1 && a->W >= 1 && a->H <= (1 << 24) && a->W <= (1 << 24),
                "mnr_tsdf_integrate: images of [%d, %d]: both sides must lie in 1 .. 2^24", a->H, a->W);
  MNR_CHECK_ARG((a->rgb != nullptr) == (a->color != nullptr), "mnr_tsdf_integrate: rgb and color are both given or both NULL");
  const int64_t nbi = (a->nx + TSDF_BI - 1) / TSDF_BI, nbj = (a->ny + TSDF_BJ - 1) / TSDF_BJ, nbk = (a->nz + TSDF_BK - 1) / TSDF_BK;
  const int64_t bricks = nbi * nbj * nbk;
  MNR_CHECK_ARG(bricks < (1ll << 31), "mnr_tsdf_integrate: a grid of [%d, %d, %d] points is too large", a->nx,
                a->ny, a->nz);
  if (a->F == 0) return MNR_OK;
  MNR_CHECK_ARG(a->proj && a->depth, "mnr_tsdf_integrate: needs proj [F,3,4] and depth [F,H,W]");
  const size_t image = (size_t)a->H * (size_t)a->W;
  for (int f0 = 0; f0 < a->F; f0 += MNR_TSDF_MAX_FRAMES) {
    mnr_tsdf_args b = *a;
    b.F = a->F - f0 < MNR_TSDF_MAX_FRAMES ? a->F - f0 : MNR_TSDF_MAX_FRAMES;
    b.proj = a->proj + (size_t)f0 * 12;
    b.depth = a->depth + (size_t)f0 * image;
    b.acc = a->acc ? a->acc + (size_t)f0 * image : nullptr;
    b.rgb = a->rgb ? a->rgb + (size_t)f0 * image * 3 : nullptr;
    const dim3 grid((unsigned)bricks), block(TSDF_THREADS);
    if (a->color != nullptr) hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, block, 0, (hipStream_t)stream, b, (int)nbj, (int)nbk);
    else hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, block, 0, (hipStream_t)stream, b, (int)nbj, (int)nbk);
    MNR_CHECK_LAUNCH();
  }
  return MNR_OK;
}

// ---- validity of the marching-tetrahedra vertices

__global__ __launch_bounds__(TSDF_THREADS) void mt_vertex_valid_kernel(mnr_mt_args a, const unsigned char* __restrict__ valid,
                                                                       unsigned char* __restrict__ keep, int64_t n_points) {
  const int64_t p = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (p >= n_points) return;
  const int64_t ij = p / a.nz;
  const int k = (int)(p - ij * a.nz), i = (int)(ij / a.ny), j = (int)(ij - (int64_t)i * a.ny);
  // (as mt_emit_vertices_kernel: mask bits of edges that leave the grid are ignored, nothing is written at or beyond n_verts)
  const unsigned ex = i + 1 < a.nx ? 1u : 0u, ey = j + 1 < a.ny ? 1u : 0u, ez = k + 1 < a.nz ? 1u : 0u;
  const unsigned in_grid = ex | (ey << 1) | (ez << 2) | ((ex & ey) << 3) | ((ex & ez) << 4) | ((ey & ez) << 5) | ((ex & ey & ez) << 6);
  const unsigned mask = a.mask[p] & in_grid;
  if (mask == 0) return;
  int64_t id = a.base[p];
  const bool v0 = valid[p] != 0;
  for (unsigned e = 0; e < 7; ++e) {
    if (!((mask >> e) & 1)) continue;
    if (id < 0 || id >= a.n_verts) return;
    const unsigned c = (0x7653421u >> (4 * e)) & 7u;        // edge number -> direction bits (x = 1, y = 2, z = 4)
    const int64_t p1 = p + (int64_t)(c & 1) * a.ny * a.nz + (int64_t)((c >> 1) & 1) * a.nz + (int64_t)((c >> 2) & 1);
    keep[id] = (v0 && valid[p1] != 0) ? 1 : 0;
    ++id;
  }
}

extern "C" int mnr_mt_vertex_valid(const mnr_mt_args* a, const unsigned char* valid, unsigned char* keep, void* stream) {
  MNR_CHECK_ARG(a && a->mask && a->base, "mnr_mt_vertex_valid: needs the mask and base [points] of the emit passes");
  MNR_CHECK_ARG(a->nx >= 2 && a->ny >= 2 && a->nz >= 2, "mnr_mt_vertex_valid: every grid dimension must be at least 2, got [%d, %d, %d]",
                a->nx, a->ny, a->nz);
  const int64_t n = (int64_t)a->nx * a->ny * a->nz, wgs = (n + TSDF_THREADS - 1) / TSDF_THREADS;
  MNR_CHECK_ARG(wgs < (1ll << 31), "mnr_mt_vertex_valid: a grid of [%d, %d, %d] points is too large", a->nx, a->ny, a->nz);
  MNR_CHECK_ARG(a->n_verts >= 0 && a->n_verts < (1ll << 31), "mnr_mt_vertex_valid: %lld vertices, must be below 2^31", (long long)a->n_verts);
  MNR_CHECK_ARG(valid, "mnr_mt_vertex_valid: needs valid [points]");
  if (a->n_verts == 0) return MNR_OK;
  MNR_CHECK_ARG(keep, "mnr_mt_vertex_valid: needs keep [n_verts]");
  hipLaunchKernelGGL(mt_vertex_valid_kernel, dim3((unsigned)wgs), dim3(TSDF_THREADS), 0, (hipStream_t)stream, *a, valid, keep, n);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---- any camera model (the header's "mnr_tsdf_integrate_cam")

#include "camera_project.h"                                 // cam_project: the forward camera model

// true when every voxel of the brick with the corner coordinates cx / cy / cz [2] skips the frame of record `rec`
template <int MODEL>
__device__ __forceinline__ bool tsdf_brick_misses_cam(const float* rec, const float* cx, const float* cy, const float* cz) {
  if (MODEL == MNR_CAM_PANO) return false;
  const float ax = fmaxf(fabsf(cx[0]), fabsf(cx[1])), ay = fmaxf(fabsf(cy[0]), fabsf(cy[1])), az = fmaxf(fabsf(cz[0]), fabsf(cz[1]));
  float mag = 0.f, mag2 = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float* M = rec + CAMP_M + 4 * r;
    mag2 = ((fabsf(M[0]) * ax + fabsf(M[1]) * ay) + fabsf(M[2]) * az) + fabsf(M[3]);
    mag = fmaxf(mag, mag2);
  }
  if (MODEL == MNR_CAM_PERSPECTIVE) {
    bool behind = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) behind = behind && camp_row(rec, 2, cx[c & 1], cy[(c >> 1) & 1], cz[(c >> 2) & 1]) < -1e-6f * mag2;
    if (behind) return true;
  }
  const float mx = 0.5f * (cx[0] + cx[1]), my = 0.5f * (cy[0] + cy[1]), mz = 0.5f * (cz[0] + cz[1]);
  const float dx = cx[1] - cx[0], dy = cy[1] - cy[0], dz = cz[1] - cz[0];
  const float rho = 1.01f * (0.5f * sqrtf((dx * dx + dy * dy) + dz * dz)) + 1e-5f * mag;
  const float m0 = camp_row(rec, 0, mx, my, mz), m1 = camp_row(rec, 1, mx, my, mz), m2 = camp_row(rec, 2, mx, my, mz);
  const float h = sqrtf(m0 * m0 + m1 * m1), D = sqrtf((m0 * m0 + m1 * m1) + m2 * m2);
  if (!(D > rho)) return false;
  const float A = atan2f(h, m2), beta = asinf(rho / D);
  const float root = sqrtf(rec[CAMP_R2MAX]);
  const float alpha_max = MODEL == MNR_CAM_PERSPECTIVE ? atanf(root) : root;
  return A - beta > alpha_max + 1e-3f;
}

template <int MODEL, bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_cam_kernel(mnr_tsdf_cam_args a, int nbj, int nbk) {
  __shared__ float l_rec[MNR_TSDF_MAX_FRAMES * MNR_CAM_REC];
  __shared__ int l_list[MNR_TSDF_MAX_FRAMES];
  __shared__ int l_count;
  const int t = threadIdx.x;
  for (int n = t; n < a.F * MNR_CAM_REC; n += TSDF_THREADS) l_rec[n] = a.cameras[n];

  const unsigned b = blockIdx.x, bij = b / (unsigned)nbk;
  const int bk = (int)(b - bij * (unsigned)nbk), bi = (int)(bij / (unsigned)nbj), bj = (int)(bij - (unsigned)bi * (unsigned)nbj);
  const int i = bi * TSDF_BI + (t >> 6), j = bj * TSDF_BJ + ((t >> 3) & 7), k = bk * TSDF_BK + (t & 7);
  __syncthreads();

  const float Wf = (float)a.W, Hf = (float)a.H;
  if (t < 64) {                                             // wave 0, one frame a lane
    bool keep = false;
    if (t < a.F) {
      const float* rec = l_rec + MNR_CAM_REC * t;
      const int ie = bi * TSDF_BI + TSDF_BI - 1, je = bj * TSDF_BJ + TSDF_BJ - 1, ke = bk * TSDF_BK + TSDF_BK - 1;
      const int i1 = ie < a.nx ? ie : a.nx - 1, j1 = je < a.ny ? je : a.ny - 1, k1 = ke < a.nz ? ke : a.nz - 1;
      const float cx[2] = {a.origin[0] + a.spacing * (float)(bi * TSDF_BI), a.origin[0] + a.spacing * (float)i1};
      const float cy[2] = {a.origin[1] + a.spacing * (float)(bj * TSDF_BJ), a.origin[1] + a.spacing * (float)j1};
      const float cz[2] = {a.origin[2] + a.spacing * (float)(bk * TSDF_BK), a.origin[2] + a.spacing * (float)k1};
      // (a record of another model or image size is not this launch's: skipped as a whole)
      keep = rec[CAMP_MODEL] == (float)MODEL && rec[CAMP_H] == Hf && rec[CAMP_W] == Wf && !tsdf_brick_misses_cam<MODEL>(rec, cx, cy, cz);
    }
    const unsigned long long bal = __ballot(keep);
    if (keep) l_list[__popcll(bal & ((1ull << t) - 1ull))] = t;
    if (t == 0) l_count = __popcll(bal);
  }
  __syncthreads();
  const int count = l_count;
  if (!(i < a.nx && j < a.ny && k < a.nz)) return;

  const float x = a.origin[0] + a.spacing * (float)i, y = a.origin[1] + a.spacing * (float)j, z = a.origin[2] + a.spacing * (float)k;
  const size_t image = (size_t)a.H * (size_t)a.W;
  float sum_t = 0.f, sum_w = 0.f, sum_c[3] = {0.f, 0.f, 0.f};
  for (int n = 0; n < count; ++n) {
    const int f = l_list[n];
    float u, v, s;
    if (!cam_project<MODEL>(l_rec + MNR_CAM_REC * f, Hf, Wf, x, y, z, u, v, s)) continue;
    if (!cam_on_image(u, v, Hf, Wf)) continue;
    const size_t pix = (size_t)f * image + (size_t)(int)v * (size_t)a.W + (size_t)(int)u;
    float obs;
    if (a.acc != nullptr && a.acc[pix] < a.acc_threshold) {
      obs = 1.f;
    } else {
      const float d = a.depth[pix];
      if (!(d > 0.f && d < TSDF_INF)) continue;
      const float e = d - s;
      if (e < -a.trunc) continue;
      obs = e / a.trunc;
      obs = obs < 1.f ? obs : 1.f;
    }
    sum_t += obs;
    sum_w += 1.f;
    if (COLOR) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sum_c[c] += a.rgb[pix * 3 + c];
    }
  }
  if (!(sum_w > 0.f)) return;
  const int64_t p = ((int64_t)i * a.ny + j) * a.nz + k;
  const float W0 = a.weight[p], Wn = W0 + sum_w;
  a.tsdf[p] = (W0 * a.tsdf[p] + sum_t) / Wn;
  if (COLOR) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.color[p * 3 + c] = (W0 * a.color[p * 3 + c] + sum_c[c]) / Wn;
  }
  a.weight[p] = Wn;
}

template <int MODEL>
static void tsdf_launch_cam(const mnr_tsdf_cam_args& b, int64_t bricks, int nbj, int nbk, void* stream) {
  const dim3 grid((unsigned)bricks), block(TSDF_THREADS);
  if (b.color != nullptr) hipLaunchKernelGGL((tsdf_integrate_cam_kernel<MODEL, true>), grid, block, 0, (hipStream_t)stream, b, nbj, nbk);
  else hipLaunchKernelGGL((tsdf_integrate_cam_kernel<MODEL, false>), grid, block, 0, (hipStream_t)stream, b, nbj, nbk);
}

extern "C" int mnr_tsdf_integrate_cam(const mnr_tsdf_cam_args* a, void* stream) {
  MNR_CHECK_ARG(a && a->tsdf && a->weight, "mnr_tsdf_integrate_cam: needs the tsdf and weight volumes");
  MNR_CHECK_ARG(a->nx >= 1 && a->ny >= 1 && a->nz >= 1, "mnr_tsdf_integrate_cam: every grid dimension must be at least 1, got [%d, %d, %d]",
                a->nx, a->ny, a->nz);
  MNR_CHECK_ARG(a->spacing > 0.f && a->spacing <= MNR_F32_MAX, "mnr_tsdf_integrate_cam: the spacing must be positive and finite, is %g",
                (double)a->spacing);
  MNR_CHECK_ARG(a->trunc > 0.f && a->trunc <= MNR_F32_MAX, "mnr_tsdf_integrate_cam: trunc must be positive and finite, is %g", (double)a->trunc);
  for (int d = 0; d < 3; ++d) MNR_CHECK_ARG(mesh_finite(a->origin[d]), "mnr_tsdf_integrate_cam: the origin must be finite");
  MNR_CHECK_ARG(a->F >= 0, "mnr_tsdf_integrate_cam: F = %d frames", a->F);
  MNR_CHECK_ARG(a->H >= 1 && a->W >= 1 && a->H <= (1 << 24) && a->W <= (1 << 24),
                "mnr_tsdf_integrate_cam: images of [%d, %d]: both sides must lie in 1 .. 2^24", a->H, a->W);
  MNR_CHECK_ARG(a->model == MNR_CAM_PERSPECTIVE || a->model == MNR_CAM_FISHEYE || a->model == MNR_CAM_PANO,
                "mnr_tsdf_integrate_cam: model = %d: must be 0 (perspective), 1 (fisheye) or 2 (pano)", a->model);
  MNR_CHECK_ARG((a->rgb != nullptr) == (a->color != nullptr), "mnr_tsdf_integrate_cam: rgb and color are both given or both NULL");
  const int64_t nbi = (a->nx + TSDF_BI - 1) / TSDF_BI, nbj = (a->ny + TSDF_BJ - 1) / TSDF_BJ, nbk = (a->nz + TSDF_BK - 1) / TSDF_BK;
  const int64_t bricks = nbi * nbj * nbk;
  MNR_CHECK_ARG(bricks < (1ll << 31), "mnr_tsdf_integrate_cam: a grid of [%d, %d, %d] points is too large", a->nx, a->ny, a->nz);
  if (a->F == 0) return MNR_OK;
  MNR_CHECK_ARG(a->cameras && a->depth, "mnr_tsdf_integrate_cam: needs cameras [F,%d] and depth [F,H,W]", MNR_CAM_REC);
  const size_t image = (size_t)a->H * (size_t)a->W;
  for (int f0 = 0; f0 < a->F; f0 += MNR_TSDF_MAX_FRAMES) {
    mnr_tsdf_cam_args b = *a;
    b.F = a->F - f0 < MNR_TSDF_MAX_FRAMES ? a->F - f0 : MNR_TSDF_MAX_FRAMES;
    b.cameras = a->cameras + (size_t)f0 * MNR_CAM_REC;
    b.depth = a->depth + (size_t)f0 * image;
    b.acc = a->acc ? a->acc + (size_t)f0 * image : nullptr;
    b.rgb = a->rgb ? a->rgb + (size_t)f0 * image * 3 : nullptr;
    if (a->model == MNR_CAM_PANO) tsdf_launch_cam<MNR_CAM_PANO>(b, bricks, (int)nbj, (int)nbk, stream);
    else if (a->model == MNR_CAM_FISHEYE) tsdf_launch_cam<MNR_CAM_FISHEYE>(b, bricks, (int)nbj, (int)nbk, stream);
    else tsdf_launch_cam<MNR_CAM_PERSPECTIVE>(b, bricks, (int)nbj, (int)nbk, stream);
    MNR_CHECK_LAUNCH();
  }
  return MNR_OK;
}
