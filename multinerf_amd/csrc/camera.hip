// Pixel -> ray generation on device (replaces camera_utils.pixels_to_rays / cast_ray_batch,
// internal/camera_utils.py:520-688, enabled by Config.cast_rays_in_train_step, train_utils.py:267-268).
// One thread per pixel: three pixel directions (centre, +x, +y) through the inverse intrinsics, optional
// radial/tangential undistortion (10 Newton steps, camera_utils.py:477-511), optional fisheye mapping,
// OpenCV -> OpenGL flip, camera rotation, optional NDC projection (camera_utils.py:32-98), cone radii.
// fp32 throughout, FP contraction off so that the arithmetic follows the reference's operation order.

#include "common.h"
#include "camera_project.h"                                 // the forward model: mnr_project_points at the end of this file

#pragma clang fp contract(off)

struct CamDist {
  float k1, k2, k3, k4, p1, p2;
};

__device__ __forceinline__ void cam_undistort(const CamDist& c, float xd, float yd, float& xo, float& yo) {
  float x = xd, y = yd;
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.0f + r * (c.k1 + r * (c.k2 + r * (c.k3 + r * c.k4)));
    const float fx = d * x + 2.0f * c.p1 * x * y + c.p2 * (r + 2.0f * x * x) - xd;
    const float fy = d * y + 2.0f * c.p2 * x * y + c.p1 * (r + 2.0f * y * y) - yd;
    const float d_r = c.k1 + r * (2.0f * c.k2 + r * (3.0f * c.k3 + r * 4.0f * c.k4));
    const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
    const float fx_x = d + d_x * x + 2.0f * c.p1 * y + 6.0f * c.p2 * x;
    const float fx_y = d_y * x + 2.0f * c.p1 * x + 2.0f * c.p2 * y;
    const float fy_x = d_x * y + 2.0f * c.p2 * y + 2.0f * c.p1 * x;
    const float fy_y = d + d_y * y + 2.0f * c.p2 * x + 6.0f * c.p1 * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const float xn = fx * fy_y - fy * fx_y;
    const float yn = fy * fx_x - fx * fy_x;
    const bool ok = fabsf(den) > 1e-9f;
    x += ok ? xn / den : 0.0f;
    y += ok ? yn / den : 0.0f;
  }
  xo = x;
  yo = y;
}

// camera_utils.py:76-98 with near = 1.
__device__ __forceinline__ void cam_to_ndc(const float* __restrict__ pndc, const float o[3], const float d[3],
                                           float on[3], float dn[3]) {
  const float t = -(1.0f + o[2]) / d[2];
  const float ox = o[0] + t * d[0], oy = o[1] + t * d[1], oz = o[2] + t * d[2];
  const float xm = 1.0f / pndc[2], ym = 1.0f / pndc[5];
  on[0] = xm * ox / oz;
  on[1] = ym * oy / oz;
  on[2] = -1.0f;
  dn[0] = xm * d[0] / d[2] - on[0];
  dn[1] = ym * d[1] / d[2] - on[1];
  dn[2] = 1.0f - on[2];
}

__global__ void pixels_to_rays_kernel(int64_t B, const int32_t* __restrict__ pix_x, const int32_t* __restrict__ pix_y,
                                      const int32_t* __restrict__ cam_idx, int num_cams,
                                      const float* __restrict__ pixtocams, const float* __restrict__ camtoworlds,
                                      int has_dist, CamDist dist, const float* __restrict__ pixtocam_ndc, int fisheye,
                                      float* __restrict__ origins, float* __restrict__ directions,
                                      float* __restrict__ viewdirs, float* __restrict__ radii,
                                      float* __restrict__ imageplane) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int ci = 0;
  if (cam_idx && num_cams > 1) {
    ci = cam_idx[b];
    ci = ci < 0 ? 0 : (ci >= num_cams ? num_cams - 1 : ci);
  }
  const float* P = pixtocams + (int64_t)ci * 9;
  const float* C = camtoworlds + (int64_t)ci * 12;
  const float px = (float)pix_x[b], py = (float)pix_y[b];
  float wd[3][3];                              // world-space directions of (centre, +x, +y)
  float ip[2];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const float u = px + (s == 1 ? 1.0f : 0.0f) + 0.5f;
    const float v = py + (s == 2 ? 1.0f : 0.0f) + 0.5f;
    float c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = P[i * 3 + 0] * u + P[i * 3 + 1] * v + P[i * 3 + 2];
    if (has_dist) {
      float xu, yu;
      cam_undistort(dist, c[0], c[1], xu, yu);
      c[0] = xu;
      c[1] = yu;
      c[2] = 1.0f;
    }
    if (fisheye) {
      float theta = sqrtf(c[0] * c[0] + c[1] * c[1]);
      theta = fminf(3.14159265358979323846f, theta);
      const float sot = sinf(theta) / theta;
      c[0] *= sot;
      c[1] *= sot;
      c[2] = cosf(theta);
    }
    c[1] = -c[1];                              // OpenCV -> OpenGL
    c[2] = -c[2];
    if (s == 0) {
      ip[0] = c[0];
      ip[1] = c[1];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) wd[s][i] = C[i * 4 + 0] * c[0] + C[i * 4 + 1] * c[1] + C[i * 4 + 2] * c[2];
  }
  float o[3] = {C[3], C[7], C[11]};
  float d[3] = {wd[0][0], wd[0][1], wd[0][2]};
  const float inv = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const float vd[3] = {d[0] * inv, d[1] * inv, d[2] * inv};
  float dxn, dyn;
  if (!pixtocam_ndc) {
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float ex = wd[1][i] - d[i], ey = wd[2][i] - d[i];
      sx += ex * ex;
      sy += ey * ey;
    }
    dxn = sqrtf(sx);
    dyn = sqrtf(sy);
  } else {
    float on[3], dn[3], ox[3], oy[3], tmp[3];
    cam_to_ndc(pixtocam_ndc, o, wd[1], ox, tmp);
    cam_to_ndc(pixtocam_ndc, o, wd[2], oy, tmp);
    cam_to_ndc(pixtocam_ndc, o, d, on, dn);
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float ex = ox[i] - on[i], ey = oy[i] - on[i];
      sx += ex * ex;
      sy += ey * ey;
      o[i] = on[i];
      d[i] = dn[i];
    }
    dxn = sqrtf(sx);
    dyn = sqrtf(sy);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    origins[b * 3 + i] = o[i];
    directions[b * 3 + i] = d[i];
    viewdirs[b * 3 + i] = vd[i];
  }
  radii[b] = (0.5f * (dxn + dyn)) * 2.0f / sqrtf(12.0f);
  imageplane[b * 2 + 0] = ip[0];
  imageplane[b * 2 + 1] = ip[1];
}

extern "C" int mnr_pixels_to_rays(int64_t B, const int32_t* pix_x_int, const int32_t* pix_y_int, const int32_t* cam_idx,
                                  int num_cams, const float* pixtocams, const float* camtoworlds,
                                  const float* distortion6, const float* pixtocam_ndc, int camtype, float* origins,
                                  float* directions, float* viewdirs, float* radii, float* imageplane, void* stream) {
  MNR_CHECK_ARG(B > 0 && pix_x_int && pix_y_int && pixtocams && camtoworlds && origins && directions && viewdirs &&
                    radii && imageplane,
                "mnr_pixels_to_rays: null argument");
  MNR_CHECK_ARG(num_cams >= 1 && (num_cams == 1 || cam_idx), "mnr_pixels_to_rays: stacked cameras need cam_idx");
  MNR_CHECK_ARG(camtype == MNR_CAM_PERSPECTIVE || camtype == MNR_CAM_FISHEYE, "mnr_pixels_to_rays: unknown camtype %d", camtype);
  CamDist dist = {0, 0, 0, 0, 0, 0};
  if (distortion6) {
    // host copy of six floats: the distortion parameters are a Python dict of floats in the reference
    dist = {distortion6[0], distortion6[1], distortion6[2], distortion6[3], distortion6[4], distortion6[5]};
  }
  hipLaunchKernelGGL(pixels_to_rays_kernel, dim3(mnr_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, B, pix_x_int,
                     pix_y_int, cam_idx, num_cams, pixtocams, camtoworlds, distortion6 ? 1 : 0, dist, pixtocam_ndc,
                     camtype == MNR_CAM_FISHEYE, origins, directions, viewdirs, radii, imageplane);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// Spherical camera (camera_utils.py:716-764).  |dx| is a difference of nearby unit vectors: in float32 it would lose
// log10(W / 6) digits, so the three grid directions are formed in float64 and every output is rounded once.
__device__ __forceinline__ void sph_direction(const double R[9], int h, int w, int H, int W, double d[3]) {
  const double two_pi = 6.283185307179586476925286766559, pi = 3.141592653589793238462643383279;
  const double theta = w == W ? two_pi : (double)w * (two_pi / (double)W);       // np.linspace: i * step, the end point exact
  const double phi = h == H ? pi : (double)h * (pi / (double)H);
  const double c[3] = {-sin(phi) * sin(theta), cos(phi), sin(phi) * cos(theta)};
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = R[i * 3 + 0] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2];
}

__global__ void spherical_rays_kernel(int H, int W, const float* __restrict__ camtoworld, float* __restrict__ origins,
                                      float* __restrict__ directions, float* __restrict__ viewdirs, float* __restrict__ radii,
                                      float* __restrict__ imageplane) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (int64_t)H * W) return;
  const int h = (int)(b / W), w = (int)(b - (int64_t)h * W);
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (double)camtoworld[i * 4 + j];
  }
  double d[3], dx[3], dy[3];
  sph_direction(R, h, w, H, W, d);
  sph_direction(R, h, w + 1, H, W, dx);
  sph_direction(R, h + 1, w, H, W, dy);
  double sx = 0.0, sy = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double ex = dx[i] - d[i], ey = dy[i] - d[i];
    sx += ex * ex;
    sy += ey * ey;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    origins[b * 3 + i] = camtoworld[i * 4 + 3];
    directions[b * 3 + i] = (float)d[i];
    viewdirs[b * 3 + i] = (float)d[i];
  }
  radii[b] = (float)((0.5 * (sqrt(sx) + sqrt(sy))) * 2.0 / sqrt(12.0));
  imageplane[b * 2 + 0] = 0.0f;
  imageplane[b * 2 + 1] = 0.0f;
}

extern "C" int mnr_spherical_rays(int H, int W, const float* camtoworld, float* origins, float* directions, float* viewdirs,
                                  float* radii, float* imageplane, void* stream) {
  MNR_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W * 3 < (1ll << 31), "mnr_spherical_rays: bad image shape [%d, %d]", H, W);
  MNR_CHECK_ARG(camtoworld && origins && directions && viewdirs && radii && imageplane, "mnr_spherical_rays: null argument");
  hipLaunchKernelGGL(spherical_rays_kernel, dim3(mnr_cdiv((int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, H, W, camtoworld,
                     origins, directions, viewdirs, radii, imageplane);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}

// ---- world point -> pixel (camera_project.h; include/mnerf.h states every operation).  One thread a point, one record a call:
// the record travels as a kernel argument, so every lane reads it from scalar registers.
struct CamRecord {
  float v[MNR_CAM_REC];
};

template <int MODEL>
__global__ __launch_bounds__(256) void project_points_kernel(int64_t n, const float* __restrict__ points, CamRecord rec, float* __restrict__ uv,
                                                            float* __restrict__ s_out, unsigned char* __restrict__ valid) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const float Hf = rec.v[CAMP_H], Wf = rec.v[CAMP_W];
  float u, v, s;
  const bool ok = cam_project<MODEL>(rec.v, Hf, Wf, points[b * 3 + 0], points[b * 3 + 1], points[b * 3 + 2], u, v, s);
  uv[b * 2 + 0] = u;
  uv[b * 2 + 1] = v;
  s_out[b] = s;
  valid[b] = (ok && cam_on_image(u, v, Hf, Wf)) ? 1 : 0;
}

extern "C" int mnr_project_points(int64_t n, const float* points, const float* record, float* uv, float* s, unsigned char* valid, void* stream) {
  MNR_CHECK_ARG(n >= 0 && n < (1ll << 31), "mnr_project_points: n = %lld points: must lie in 0 .. 2^31 - 1", (long long)n);
  MNR_CHECK_ARG(record, "mnr_project_points: needs the camera record (%d floats, a host pointer)", MNR_CAM_REC);
  CamRecord rec;
  for (int i = 0; i < MNR_CAM_REC; ++i) rec.v[i] = record[i];
  const float model = rec.v[CAMP_MODEL];
  MNR_CHECK_ARG(model == (float)MNR_CAM_PERSPECTIVE || model == (float)MNR_CAM_FISHEYE || model == (float)MNR_CAM_PANO,
                "mnr_project_points: the record's model is %g: must be 0 (perspective), 1 (fisheye) or 2 (pano)", (double)model);
  MNR_CHECK_ARG(rec.v[CAMP_H] >= 1.f && rec.v[CAMP_W] >= 1.f && rec.v[CAMP_H] <= 16777216.f && rec.v[CAMP_W] <= 16777216.f,
                "mnr_project_points: the record's image is [%g, %g]: both sides must lie in 1 .. 2^24", (double)rec.v[CAMP_H], (double)rec.v[CAMP_W]);
  if (n == 0) return MNR_OK;
  MNR_CHECK_ARG(points && uv && s && valid, "mnr_project_points: needs points [n,3], uv [n,2], s [n] and valid [n]");
  const dim3 grid(mnr_cdiv(n, 256)), block(256);
  if (model == (float)MNR_CAM_PANO)
    hipLaunchKernelGGL(project_points_kernel<MNR_CAM_PANO>, grid, block, 0, (hipStream_t)stream, n, points, rec, uv, s, valid);
  else if (model == (float)MNR_CAM_FISHEYE)
    hipLaunchKernelGGL(project_points_kernel<MNR_CAM_FISHEYE>, grid, block, 0, (hipStream_t)stream, n, points, rec, uv, s, valid);
  else
    hipLaunchKernelGGL(project_points_kernel<MNR_CAM_PERSPECTIVE>, grid, block, 0, (hipStream_t)stream, n, points, rec, uv, s, valid);
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
