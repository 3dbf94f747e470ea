// World point -> pixel: the forward camera model (include/mnerf.h, "The forward camera model", states every operation), for
// mnr_project_points (camera.hip) and mnr_tsdf_integrate_cam (tsdf.hip).
//
// It is camera.hip read backwards.  pixels_to_rays_kernel takes a pixel centre through pixtocam, undistorts it (cam_undistort: the
// Newton iteration that solves distort(x, y) = (xd, yd)), bends it for a fisheye lens (theta = |(x, y)|, direction
// (sin theta (x, y) / theta, cos theta)), flips OpenCV -> OpenGL and rotates with R.  So here: rotate back and flip
// (M = diag(1,-1,-1) [R^T | -R^T o]), un-bend (theta = atan2(h, c_z)), DISTORT, which is the closed form cam_undistort inverts,
// and apply the first two rows of inv(pixtocam).  spherical_rays_kernel's direction is R (-sin phi sin theta, cos phi,
// sin phi cos theta): phi and theta are read off R^T (X - o) / |X - o|.
//
// The returned s is the ray parameter of the point along that pixel's `directions`: the undistorted perspective direction has
// camera-space z = 1 (pixtocam's last row is (0, 0, 1) and cam_undistort sets c[2] = 1), so s = c_z; the fisheye and spherical
// directions have unit length, so s = |c|.
//
// float32 in the order written; the pragma is here for the reason mesh_math.h gives.
#pragma once

#include "common.h"

#pragma clang fp contract(off)

#define CAMP_M 0
#define CAMP_A 12
#define CAMP_K 18
#define CAMP_R2MAX 24
#define CAMP_MODEL 25
#define CAMP_H 26
#define CAMP_W 27

static_assert(MNR_CAM_REC == 28, "the record layout of include/mnerf.h");

// c_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]
__device__ __forceinline__ float camp_row(const float* rec, int r, float x, float y, float z) {
  const float* M = rec + CAMP_M + 4 * r;
  return ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
}

// (u, v, s) of the world point (x, y, z) seen by the camera record `rec` in an image of Hf x Wf pixels; the return value is `ok`:
// the point is in front of the model and inside the fold-back guard.  Whether (u, v) lies on the image is the caller's test.
template <int MODEL>
__device__ __forceinline__ bool cam_project(const float* rec, float Hf, float Wf, float x, float y, float z, float& u, float& v, float& s) {
  const float c0 = camp_row(rec, 0, x, y, z), c1 = camp_row(rec, 1, x, y, z), c2 = camp_row(rec, 2, x, y, z);
  if (MODEL == MNR_CAM_PANO) {
    s = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    const float ny = fminf(1.0f, fmaxf(-1.0f, -c1 / s));
    const float phi = acosf(ny);
    float theta = atan2f(-c0, -c2);
    if (theta < 0.0f) theta = theta + 6.2831855f;
    u = theta * Wf / 6.2831855f + 0.5f;
    if (u >= Wf) u = u - Wf;
    v = phi * Hf / 3.1415927f + 0.5f;
    if (v >= Hf) v = Hf - 0.5f;
    return s > 0.0f && s < __builtin_huge_valf();
  }
  float X, Y;
  bool ok;
  if (MODEL == MNR_CAM_FISHEYE) {
    const float h2 = c0 * c0 + c1 * c1;
    const float h = sqrtf(h2);
    const float theta = atan2f(h, c2);
    const float q = h > 0.0f ? theta / h : 0.0f;
    X = q * c0;
    Y = q * c1;
    s = sqrtf(h2 + c2 * c2);
    ok = theta * theta <= rec[CAMP_R2MAX] && (h > 0.0f || c2 > 0.0f);
  } else {
    X = c0 / c2;
    Y = c1 / c2;
    s = c2;
    ok = c2 > 0.0f;
  }
  const float r = X * X + Y * Y;
  if (MODEL == MNR_CAM_PERSPECTIVE) ok = ok && r <= rec[CAMP_R2MAX];
  const float* k = rec + CAMP_K;                            // k1, k2, k3, k4, p1, p2
  const float d = 1.0f + r * (k[0] + r * (k[1] + r * (k[2] + r * k[3])));
  const float xd = d * X + 2.0f * k[4] * X * Y + k[5] * (r + 2.0f * X * X);
  const float yd = d * Y + 2.0f * k[5] * X * Y + k[4] * (r + 2.0f * Y * Y);
  const float* a = rec + CAMP_A;
  u = (a[0] * xd + a[1] * yd) + a[2];
  v = (a[3] * xd + a[4] * yd) + a[5];
  return ok;
}

// pixel px covers [px, px + 1); false for a NaN
__device__ __forceinline__ bool cam_on_image(float u, float v, float Hf, float Wf) { return u >= 0.0f && u < Wf && v >= 0.0f && v < Hf; }
