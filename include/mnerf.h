/* mnerf.h -- C ABI of libmnerf_hip.so: MI355X (gfx950) kernels for the MultiNeRF
 * per-ray render/train hot path.
 *
 * The reference (google-research/multinerf) is pure Python/JAX and has no
 * native operator interface; its hot path is the Python call surface
 * Model.__call__ / MLP.__call__ / train_step.  This header is the boundary a
 * host (ctypes here; cffi/pybind in a maintainer's tree)
 * binds to replace the jax.numpy bodies of those functions.  Each entry point
 * names the reference function(s) it replaces (file:line under the reference
 * repository root).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (row-major,
 *    contiguous unless a leading dimension is given); the library never
 *    allocates, frees or retains them;
 *  - `stream` is a hipStream_t passed as void*; calls only enqueue work;
 *  - return value: 0 (MNR_OK) or a negative mnr_status; mnr_last_error()
 *    returns a thread-local NUL-terminated description of the last failure;
 *  - fp32 unless a name says bf16 (raw IEEE bfloat16, uint16_t storage);
 *  - "B" = rays, "n" = intervals along a ray, fence-post arrays have n+1
 *    entries (reference internal/stepfun.py:15-23).
 */
#ifndef MNERF_H_
#define MNERF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MNR_OK = 0,
  MNR_ERR_INVALID_ARGUMENT = -1,
  MNR_ERR_HIP = -2,
  MNR_ERR_UNSUPPORTED = -3
} mnr_status;

const char* mnr_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int mnr_abi_version(void);
/* Device properties the host needs to size launches: fills cu_count, lds_bytes, gcn arch name. */
int mnr_device_info(int device, int* cu_count, int* lds_bytes_per_cu, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------- *
 * Sampling  (replaces models.py:153-204 = stepfun.max_dilate_weights
 * stepfun.py:99-128, anneal/logits models.py:173-185, stepfun.sample_intervals
 * stepfun.py:164-263 incl. invert_cdf :153-161, integrate_weights :131-150,
 * math.sorted_interp math.py:108-127, and coord.construct_ray_warps s_to_t
 * coord.py:63-99)
 * ------------------------------------------------------------------------- */
typedef enum { MNR_RAYDIST_IDENTITY = 0, MNR_RAYDIST_RECIPROCAL = 1, MNR_RAYDIST_PIECEWISE = 2,
               MNR_RAYDIST_LOG = 3, MNR_RAYDIST_EXP = 4, MNR_RAYDIST_SQRT = 5, MNR_RAYDIST_SQUARE = 6 } mnr_raydist;

typedef struct {
  int n_prev;              /* intervals in the incoming step function (1 at level 0)  */
  int n_samples;           /* intervals to draw (Model.num_prop_samples / num_nerf_samples) */
  int use_dilation;        /* models.py:162-171 (level > 0 and dilation enabled)      */
  float dilation;          /* models.py:153-154                                       */
  float domain_lo, domain_hi; /* (init_s_near, init_s_far)                            */
  float anneal;            /* Schlick bias of train_frac, models.py:174-179 (1 if slope==0) */
  float resample_padding;  /* models.py:70                                            */
  int single_jitter;       /* jitter shape [B] (1) or [B,n_samples] (0)               */
  float max_jitter;        /* stepfun.py:204-205; ignored when jitter == NULL         */
  int raydist_fn;          /* mnr_raydist for s_to_t                                  */
} mnr_resample_cfg;

/* One hierarchical-sampling level for B rays.
 *  sdist_prev [B,n_prev+1], w_prev [B,n_prev]: incoming step function (s-space).
 *  u_base [n_samples]: the linspace of stepfun.py:198 / :208 (host-computed).
 *  jitter: NULL (rng=None) or uniform[0,1) draws, [B] or [B,n_samples].
 *  near,far [B].  Outputs: sdist [B,n+1], tdist [B,n+1]; idx_out (optional,
 *  may be NULL) [B,n] int32 = count(cw <= u) - 1, the bit-exact sample index. */
int mnr_resample_level(const mnr_resample_cfg* cfg, int64_t B,
                       const float* sdist_prev, const float* w_prev,
                       const float* u_base, const float* jitter,
                       const float* near, const float* far,
                       float* sdist_out, float* tdist_out, int32_t* idx_out, void* stream);

/* VJP of mnr_resample_level w.r.t. its incoming step function: Model.stop_level_grad = False (models.py:56,198-201; what
 * jax differentiates there: stepfun.max_dilate_weights stepfun.py:99-128, the logits models.py:183-185, jax.nn.softmax and
 * integrate_weights stepfun.py:131-156, math.sorted_interp math.py:108-127, the interval fence-posts stepfun.py:252-262).
 *  Inputs as the forward call's (same cfg, sdist_prev, w_prev, u_base, jitter: the forward pass is re-run inside);
 *  g_sdist [B,n+1] = d loss / d sdist_out.  Outputs (overwritten): g_sdist_prev [B,n_prev+1], g_w_prev [B,n_prev]. */
int mnr_resample_level_bwd(const mnr_resample_cfg* cfg, int64_t B,
                           const float* sdist_prev, const float* w_prev,
                           const float* u_base, const float* jitter, const float* g_sdist,
                           float* g_sdist_prev, float* g_w_prev, void* stream);

/* Leaf: math.sorted_interp(u, cw, t) (math.py:108-127) with the integer index.
 * cw,t [B,nc]; u [B,nu] -> out [B,nu], idx [B,nu] (may be NULL). */
int mnr_sorted_interp(int64_t B, int nc, int nu, const float* u, const float* cw, const float* t,
                      float* out, int32_t* idx, void* stream);

/* Leaf: stepfun.max_dilate_weights(t, w, dilation, domain, renormalize=True)
 * (stepfun.py:116-128). t [B,n+1], w [B,n] -> t_out [B,3n+1], w_out [B,3n];
 * scratch: unused since round 2 (the kernel works in LDS); kept in the signature, may be NULL. */
int mnr_max_dilate_weights(int64_t B, int n, const float* t, const float* w, float dilation,
                           float domain_lo, float domain_hi, float* t_out, float* w_out,
                           float* scratch, void* stream);

/* ------------------------------------------------------------------------- *
 * Featurisation  (replaces render.cast_rays render.py:103-127 incl.
 * conical_frustum_to_gaussian :44-78 / cylinder_to_gaussian :81-100 /
 * lift_gaussian :21-41, coord.track_linearize(coord.contract) coord.py:21-60,
 * coord.lift_and_diagonalize :129-133, coord.integrated_pos_enc :102-126 with
 * math.safe_sin math.py:26-38; and coord.pos_enc :136-147 for view directions)
 * ------------------------------------------------------------------------- */
typedef struct {
  int ray_shape;       /* 0 cone, 1 cylinder (Model.ray_shape)                */
  int warp_contract;   /* 1: MLP.warp_fn = coord.contract                     */
  int disable_integration; /* Model.disable_integration: zero covariances     */
  int basis_k;         /* K columns of pos_basis_t (21 icosa-2, 3 octa-1)     */
  int min_deg, max_deg;
} mnr_ipe_cfg;

/* tdist [B,n+1]; origins, directions [B,3]; radii [B]; basis [K,3] (rows =
 * geopoly.generate_basis rows, geopoly.py:78-124).  feat_out: bf16
 * [B*n, ld_feat], columns [0, 2*K*(max_deg-min_deg)) = IPE features in the
 * reference order, remaining columns zero.  means_out / covs_out (optional,
 * fp32 [B*n,3] / [B*n,9]) are the POST-warp Gaussians, for parity tests. */
int mnr_cast_rays_ipe(const mnr_ipe_cfg* cfg, int64_t B, int n, const float* tdist,
                      const float* origins, const float* directions, const float* radii,
                      const float* basis, uint16_t* feat_out, int ld_feat,
                      float* means_out, float* covs_out, void* stream);

/* Same, fp32 features [B*n, 2*K*L] (no padding): parity-test leaf for
 * coord.integrated_pos_enc. */
int mnr_cast_rays_ipe_f32(const mnr_ipe_cfg* cfg, int64_t B, int n, const float* tdist,
                          const float* origins, const float* directions, const float* radii,
                          const float* basis, float* feat_out, void* stream);

/* Tangent features for the density-gradient normals (models.py:478-492 via forward mode):
 * row c*B*n + s of feat_out (bf16 [3*B*n, ld_feat]) = d(IPE features of sample s)/d(mean_c), c = x,y,z, mean = the Gaussian's
 * mean as predict_density receives it (models.py:441-446: BEFORE warp_fn; with cfg->warp_contract the rows carry the
 * contraction's Jacobian and, through J cov J^T with the covariance held fixed, its derivative).
 * Rows of ld_feat <= 40 are refused (three staged rows per sample would need more than 64 KiB of LDS per block), here and in
 * mnr_ipe_from_gaussians_tangent. */
int mnr_cast_rays_ipe_tangent(const mnr_ipe_cfg* cfg, int64_t B, int n, const float* tdist,
                              const float* origins, const float* directions, const float* radii,
                              const float* basis, uint16_t* feat_out, int ld_feat, void* stream);

/* VJP of mnr_cast_rays_ipe w.r.t. the interval ends (Model.stop_level_grad = False, models.py:198-201: render.cast_rays
 * render.py:103-127 incl. the conical-frustum / cylinder moments :44-100 and lift_gaussian :21-41, coord.track_linearize(
 * contract) coord.py:21-60 with the contraction's second derivative, lift_and_diagonalize :129-133, integrated_pos_enc
 * :102-126).  g_feat_a (and optionally g_feat_b, summed) bf16 [B*n, ld_feat] = d loss / d features;
 * outputs g_t0, g_t1 fp32 [B*n] = d loss / d (tdist[ray, j], tdist[ray, j+1]) of sample (ray, j). */
int mnr_cast_rays_ipe_bwd(const mnr_ipe_cfg* cfg, int64_t B, int n, const float* tdist,
                          const float* origins, const float* directions, const float* radii,
                          const float* basis, const uint16_t* g_feat_a, const uint16_t* g_feat_b, int ld_feat,
                          float* g_t0, float* g_t1, void* stream);

/* VJP of mnr_cast_rays_ipe_tangent w.r.t. the interval ends: Model.stop_level_grad = False next to density-gradient normals
 * (models.py:198-201 with :478-492: the normals are a derivative of predict_density AT the sample's Gaussian, so they depend on
 * the sample positions as well).  g_T_a (and optionally g_T_b, summed) bf16 [3*B*n, ld_feat] = d loss / d (tangent rows) (the
 * tangent network's dX GEMMs of the trunk layers that read the features); g_t0, g_t1 fp32 [B*n] are ACCUMULATED into (call
 * after mnr_cast_rays_ipe_bwd).  With cfg->warp_contract the contraction's third derivative enters (forward-mode duals). */
int mnr_cast_rays_ipe_tangent_bwd(const mnr_ipe_cfg* cfg, int64_t B, int n, const float* tdist,
                                  const float* origins, const float* directions, const float* radii,
                                  const float* basis, const uint16_t* g_T_a, const uint16_t* g_T_b, int ld_feat,
                                  float* g_t0, float* g_t1, void* stream);

/* The featurisation of a stand-alone MLP call on CALLER-SUPPLIED Gaussians (replaces MLP.__call__'s own featurisation,
 * models.py:403-409 with predict_density's :441-449: coord.track_linearize(coord.contract) coord.py:21-60 for a GENERAL
 * covariance, lift_and_diagonalize :129-133, integrated_pos_enc :102-126 with math.safe_sin math.py:26-38).
 *  means [M,3], covs [M,9] (row-major 3x3; symmetrised as 0.5 (c_ij + c_ji)): the Gaussians BEFORE warp_fn.
 *  feat_out: bf16 [M, ld_feat] as mnr_cast_rays_ipe writes it (columns [2KL, ld_feat) zero); feat_f32_out (optional) the same
 *  features unrounded, fp32 [M, 2KL]; means_out / covs_out (optional, fp32 [M,3] / [M,9]) the POST-warp Gaussians.
 *  cfg->ray_shape and cfg->disable_integration are not read.  Behind the Gaussian the arithmetic is mnr_cast_rays_ipe's: on
 *  the Gaussians that call exports without a contraction, the rows are bit-identical. */
int mnr_ipe_from_gaussians(const mnr_ipe_cfg* cfg, int64_t M, const float* means, const float* covs,
                           const float* basis, void* feat_out, int ld_feat, float* feat_f32_out,
                           float* means_out, float* covs_out, void* stream);

/* Tangent rows of the same call (models.py:473-492 via forward mode, as mnr_cast_rays_ipe_tangent): row c*M + s of feat_out
 * (bf16 [3*M, ld_feat]) = d(IPE features of sample s)/d(mean_c), c = x,y,z, with the covariance an input held fixed; under
 * cfg->warp_contract the rows carry the contraction's Jacobian and d(J cov J^T)/d(mean_c). */
int mnr_ipe_from_gaussians_tangent(const mnr_ipe_cfg* cfg, int64_t M, const float* means, const float* covs,
                                   const float* basis, void* feat_out, int ld_feat, void* stream);

/* coord.pos_enc(viewdirs, 0, deg_view, append_identity=True) per ray, written
 * (bf16) into columns [col0, col0+3+6*deg_view) of every one of the ray's n
 * rows of `dst` [B*n, ld]; columns up to col_end are zero-filled
 * (models.py:550-557 broadcast + concat). */
int mnr_viewdir_enc_fill(int64_t B, int n, const float* viewdirs, int deg_view,
                         uint16_t* dst, int ld, int col0, int col_end, void* stream);

/* ------------------------------------------------------------------------- *
 * Ray generation  (replaces camera_utils.pixels_to_rays / cast_ray_batch,
 * internal/camera_utils.py:520-688; used when Config.cast_rays_in_train_step,
 * train_utils.py:267-268)
 * pix_x_int / pix_y_int / cam_idx: int32 [B] (device).  pixtocams [num_cams,3,3],
 * camtoworlds [num_cams,3,4] fp32 (device; num_cams == 1: one camera for all pixels,
 * cam_idx may be NULL).  distortion6 = HOST pointer to {k1,k2,k3,k4,p1,p2} or NULL.
 * pixtocam_ndc: device [3,3] or NULL (NDC rays, camera_utils.py:32-98).
 * Outputs fp32 device: origins, directions, viewdirs [B,3], radii [B], imageplane [B,2].
 * ------------------------------------------------------------------------- */
typedef enum { MNR_CAM_PERSPECTIVE = 0, MNR_CAM_FISHEYE = 1, MNR_CAM_PANO = 2 /* camera records only, see below */ } mnr_camtype;
int mnr_pixels_to_rays(int64_t B, const int32_t* pix_x_int, const int32_t* pix_y_int, const int32_t* cam_idx,
                       int num_cams, const float* pixtocams, const float* camtoworlds, const float* distortion6,
                       const float* pixtocam_ndc, int camtype, float* origins, float* directions, float* viewdirs,
                       float* radii, float* imageplane, void* stream);

/* Rays of a spherical (panorama) camera, camera_utils.cast_spherical_rays (camera_utils.py:716-764): pixel (h, w) looks
 * along the direction at theta = linspace(0, 2 pi, W + 1)[w], phi = linspace(0, pi, H + 1)[h] (y up), rotated by
 * camtoworld [3,4] (fp32, device); radii from the forward differences to (h, w + 1) and (h + 1, w).  One thread per pixel
 * recomputes its three grid directions in float64 and rounds once.  Outputs fp32 device: origins, directions, viewdirs
 * [H,W,3] (viewdirs = directions: unit already), radii [H,W], imageplane [H,W,2] = 0. */
int mnr_spherical_rays(int H, int W, const float* camtoworld, float* origins, float* directions, float* viewdirs,
                       float* radii, float* imageplane, void* stream);

/* ------------------------------------------------------------------------- *
 * The forward camera model: world point -> pixel  (csrc/camera_project.h; mnr_project_points in csrc/camera.hip,
 * mnr_tsdf_integrate_cam in csrc/tsdf.hip)
 * The inverse of the two ray generators above, for the rays in WORLD space (no NDC): a point X = origins + s directions of pixel
 * (px, py) maps to (u, v) with int(u) = px, int(v) = py, and to that s.  s is the ray parameter in units of the length of
 * `directions`, i.e. the distance a model renders along those rays: the camera-space depth for a perspective camera (the ray's
 * camera-space z is 1), the Euclidean distance for fisheye and pano (unit directions).
 *
 * A camera is a RECORD of MNR_CAM_REC = 28 floats (mesh.camera_record builds it in float64 and rounds once):
 *   [0..11]   M [3,4] = diag(1,-1,-1) [R^T | -R^T o] for camtoworld = [R | o]: world -> OpenCV camera frame
 *   [12..17]  a [2,3]: the first two rows of inv(pixtocam); the last row of pixtocam must be (0, 0, 1)
 *   [18..23]  k1, k2, k3, k4, p1, p2 (all 0: no lens distortion)
 *   [24]      r2_max, the fold-back guard (below)      [25] the model, an mnr_camtype as a float
 *   [26]      float(H)                                 [27] float(W)
 * For MNR_CAM_PANO only M, the model, H and W are read.
 *
 * Per point (x, y, z), float32 in the order written, no contraction; a comparison with a NaN is false, so ok is false:
 *   c_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3] for r = 0, 1, 2.
 *   PERSPECTIVE  ok = c_2 > 0;  X = c_0 / c_2, Y = c_1 / c_2, s = c_2;  r = X X + Y Y;  ok = ok and r <= r2_max.
 *   FISHEYE      h = sqrtf(c_0 c_0 + c_1 c_1), theta = atan2f(h, c_2), q = theta / h (0 where h == 0), X = q c_0, Y = q c_1,
 *                s = sqrtf((c_0 c_0 + c_1 c_1) + c_2 c_2);  r = X X + Y Y;  ok = theta theta <= r2_max and (h > 0 or c_2 > 0)
 *                (h == 0 and c_2 <= 0 is the eye itself or the one direction every pixel at theta = pi shares).
 *   both         d = 1 + r (k1 + r (k2 + r (k3 + r k4)));
 *                xd = (d X + ((2 p1) X) Y) + p2 (r + (2 X) X),  yd = (d Y + ((2 p2) X) Y) + p1 (r + (2 Y) Y)
 *                (cam_undistort's fx, fy without the "- xd", "- yd");
 *                u = (a00 xd + a01 yd) + a02,  v = (a10 xd + a11 yd) + a12.
 *   PANO         s = sqrtf((c_0 c_0 + c_1 c_1) + c_2 c_2);  ok = 0 < s < inf;  n_y = min(1, max(-1, -c_1 / s));
 *                phi = acosf(n_y);  theta = atan2f(-c_0, -c_2), + 6.2831855f where negative;
 *                u = theta W / 6.2831855f + 0.5f, - W where u >= W;  v = phi H / 3.1415927f + 0.5f, H - 0.5f where v >= H
 *                (mnr_spherical_rays' pixel (h, w) looks along theta = 2 pi w / W, phi = pi h / H: a grid POINT, so int(u), int(v)
 *                are the nearest grid point, column W wrapping to 0 and row H, the pole, going to row H - 1).
 *   valid = ok and 0 <= u < W and 0 <= v < H.  Pixel px covers [px, px + 1).
 * The perspective model uses only + - x / and comparisons: a NumPy float32 restatement reproduces it bit for bit.
 *
 * The fold-back guard.  The distortion polynomial is not injective: far outside the image it folds back, and a point there would
 * land inside the image, mirrored.  r2_max bounds X X + Y Y (for fisheye theta theta) to the image's own pre-image: the host
 * undistorts the pixel corners along the four image edges (Newton, float64, to convergence), takes the largest squared radius,
 * times 1.01^2 for the border between the corners, at most pi^2 for fisheye.  The radius' maximum over the pre-image lies on its
 * border, so the guard drops nothing that is in the image.
 *
 * mnr_project_points: points [n,3] (device) through ONE record (28 floats, a HOST pointer, copied at the call) ->
 * uv [n,2], s [n] float32 and valid [n] bytes (device); one thread a point.  u, v and s are written whatever valid is.
 * n == 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
#define MNR_CAM_REC 28
int mnr_project_points(int64_t n, const float* points, const float* record, float* uv, float* s, unsigned char* valid, void* stream);

/* GLO vectors (models.py:101-110,565-568): dst[b*n+i, col0+g] = table[cam_idx[b], g] (bf16), or 0 when
 * cam_idx is NULL (zero_glo=True).  table [num_embeddings, G] fp32 = params['Embed_0']['embedding']. */
int mnr_glo_fill(int64_t B, int n, int G, const float* table, const int32_t* cam_idx, int num_embeddings,
                 uint16_t* dst, int ld, int col0, void* stream);
/* VJP: grad_table[cam_idx[b], g] += sum_i (g_a[b*n+i, g] + g_b[b*n+i, g]); g_a / g_b fp32 [B*n, G] (g_b may be NULL). */
int mnr_glo_bwd(int64_t B, int n, int G, const float* g_a, const float* g_b, const int32_t* cam_idx,
                int num_embeddings, float* grad_table, void* stream);

/* ------------------------------------------------------------------------- *
 * Dense layers  (replaces flax.linen.Dense at models.py:436-437,456,460,495,
 * 515,518,521,527,577,585: y = x @ kernel[in,out] + bias, and their VJPs)
 * bf16 operands, fp32 accumulation on the MFMA units.
 * ------------------------------------------------------------------------- */
typedef struct {
  /* A = [A1 | A2] : [M, K1+K2] bf16; K1,K2 multiples of 64 (of 32 with c_layout = PANEL); A2 may be NULL (K2=0).
   * The second segment is the skip concat of models.py:458-459. */
  const uint16_t* A1; int lda1; int K1;
  const uint16_t* A2; int lda2; int K2;
  const uint16_t* Bt; int ldb;        /* [N, K1+K2] bf16: row n = output column n */
  int64_t M;                          /* multiple of 128 */
  int N;                              /* multiple of 128 (padded rows of Bt are zero) */
  const float* bias; int n_bias;      /* bias[n] added for n < n_bias (may be NULL) */
  int relu;                           /* nn.relu epilogue                          */
  const uint16_t* mask; int ldmask;   /* optional: out *= (mask[m,n] > 0)  (ReLU VJP) */
  uint16_t* Cb; int ldcb; int nb;     /* bf16 output for columns n < nb (may be NULL) */
  float* Cf; int ldcf; int f0; int nf;/* fp32 output for f0 <= n < f0+nf at column n-f0 */
  /* 1-bit ReLU masks, bit (n & 7) of byte [m*ld + n/8]: the forward layer writes (out > 0), the dX
   * GEMM of the next layer reads it instead of re-reading the bf16 activation (16x less traffic). */
  uint8_t* mask_bits_out; int ld_bits_out;
  const uint8_t* mask_bits_in; int ld_bits_in;
  int64_t bits_row_mod;               /* > 0: row m reads the bits of row m % bits_row_mod (tangent rows
                                         c*M + s share the primal mask of sample s) */
  /* Storage of the activation operand A1 and of the bf16 result (MNR_LAYOUT_*).  MNR_LAYOUT_PANEL is the layout the
   * 1024-wide trunk's activations and gradients live in between this library's own GEMMs (every producer and consumer
   * of such a matrix is a kernel of this file; the reference's per-layer tensors models.py:441-465 never leave it):
   * element (m, n) of an [M, W] matrix sits at ((m / 32) * (W / 16) + n / 16) * 512 + (m % 32) * 16 + n % 16, i.e.
   * 1-KiB blocks of 32 rows x 16 columns, which an MFMA wave writes straight from its accumulators as whole blocks
   * (no transposition through LDS) and which the next GEMM's LDS-DMA reads in 512-byte runs.  M %% 256 == 0, W %% 256 == 0.
   * With c_layout = PANEL the 1-bit ReLU masks are in TILE order: 8 KiB per 256 x 256 output tile (tile index
   * m_tile * (N / 256) + n_tile), thread t of the tile's 512 owns 16 bytes; byte (j * 4 + i) * 2 + h of thread
   * t = (wm * 4 + wn) * 64 + kh * 32 + r covers row wm * 128 + i * 32 + r, columns wn * 64 + j * 32 + h * 16 + kh * 8 .. + 7
   * of the tile (bit e = column + e); written by the forward layer, read by the dX layer of the same tile shape
   * (ld_bits_* are ignored).  Restrictions of c_layout = PANEL: K1 + K2 >= 192, no fp32 side output, no bf16 mask,
   * nb == N, forward layers carry a full bias (n_bias == N), bits_row_mod == 0; A2 and Bt are always row-major. */
  int a1_layout; int c_layout;
  /* One more output column supplied as a VECTOR: vcol_out[m] = sum_k [A1|A2][m, k] * vcol[k] + *vcol_bias (fp32), next to an
   * N = 256 result.  The NeRF MLP's density head (internal/models.py:460) next to its 256-wide bottleneck (:527): both read the
   * last trunk activation, and as column 257 of a merged operand the density would cost a second 256-column tile of MFMAs.
   * Each of the four waves that share a row block spends one extra MFMA per k-step on it (+12.5 %).  vcol: bf16 [K1 + K2]
   * (16-byte aligned); needs a1_layout = PANEL, N == 256, K1 + K2 <= 1536, a row-major bf16 result, no fp32 side output. */
  const uint16_t* vcol; float* vcol_out; const float* vcol_bias;     /* vcol_bias: one device float, or NULL for 0 */
  /* c_layout = PANEL: 1 = walk the M-tiles in descending order (the caller alternates it between consecutive layers: a layer
   * then starts with the rows the previous one wrote last).  Performance only; results do not depend on it. */
  int walk_descending;
  int max_wgs;                 /* c_layout = PANEL: > 0 caps the persistent grid (a paired launch shares the chip, see mnr_gemm_tn_args) */
} mnr_gemm_nt_args;
#define MNR_LAYOUT_ROWMAJOR 0
#define MNR_LAYOUT_PANEL 1

/* C[M,N] = epilogue([A1|A2] * Bt^T). */
int mnr_gemm_nt_bf16(const mnr_gemm_nt_args* args, void* stream);

/* ---- Fused Dense chain (csrc/fused_mlp.hip): the trunk of internal/models.py:441-465 (Dense + ReLU layers, optionally
 * one skip concat of the input features, :458-459) and, for a density-only MLP, its Dense(1) head (:460) as ONE
 * persistent kernel per sampling level; replaces depth (+ 1) mnr_gemm_nt_bf16 launches (forward) / the dX chain
 * (backward).  The activation tile of a 256-row block stays in LDS between layers; weights go global -> registers.
 * Widths 128 / 256: the proposal MLP of every config and the 256-wide NeRF MLPs of blender_256 / llff_raw / blender_refnerf. */
#define MNR_CHAIN_MAX_DEPTH 8
typedef struct {
  int64_t M;                  /* rows (samples of the level): a multiple of 256 */
  int W;                      /* layer width: 128 or 256 */
  int depth;                  /* number of Dense + ReLU layers, 1..MNR_CHAIN_MAX_DEPTH */
  const uint16_t* feat;       /* [M, ld_feat] bf16: input of layer 0 (IPE features), columns >= fan_in zero */
  int ld_feat; int K0;        /* K0 = padded fan_in of layer 0, a multiple of 64 */
  const uint16_t* Bt[MNR_CHAIN_MAX_DEPTH];   /* layer i: [W, ldb[i]] bf16 = kernel^T (row = output column) */
  int ldb[MNR_CHAIN_MAX_DEPTH];
  const float* bias[MNR_CHAIN_MAX_DEPTH];    /* [W] fp32 */
  const uint16_t* w_head;     /* [W] bf16 Dense(1) kernel applied to the last activation; NULL: no head */
  const float* b_head;        /* [1] fp32 on the device (NULL: 0) */
  float* head_out;            /* [M] fp32: x_last . w_head + b_head */
  uint16_t* acts[MNR_CHAIN_MAX_DEPTH];       /* optional out: activation of layer i, [M, W] bf16 (training: dW inputs) */
  uint8_t* bits[MNR_CHAIN_MAX_DEPTH];        /* optional out: its ReLU mask, 1 bit per element, [M, W/8] */
  int skip_layer;             /* > 0: layer `skip_layer` reads [x_{skip_layer-1} | feat] (the skip concat of models.py:458-459):
                                 Bt[skip_layer] has W + K0 columns, the feature part behind the W activation columns; 0: none */
} mnr_mlp_chain_fwd_args;
int mnr_mlp_chain_fwd(const mnr_mlp_chain_fwd_args* args, void* stream);

/* The same forward chain with layer 0's A operand PRODUCED IN THE KERNEL (inference: no per-layer outputs, no skip concat):
 * render.cast_rays (render.py:103-127), coord.track_linearize(coord.contract) (coord.py:21-60), lift_and_diagonalize
 * (:129-133) and integrated_pos_enc (:102-126) are evaluated per 256-sample tile straight into the LDS tile the MFMAs read,
 * four encoding degrees (one "group") at a time; the [M, 2KL] feature matrix of mnr_cast_rays_ipe never exists.
 * chain->feat / ld_feat / K0 are unused; acts[i] / bits[i] must be NULL except acts[depth-1]; chain->Bt[0] is layer 0's
 * kernel^T with its K columns REORDERED group-major (L = max_deg - min_deg, K = basis_k, G = MNR_CHAIN_IPE_GROUP_COLS):
 *   column g*G + dl*2K + s*K + k  =  kernel row  s*K*L + (4g+dl)*K + k     (s = 0 sin / 1 cos, dl = 0..3, k < K)
 * and columns [8K, G) of every group zero; chain->ldb[0] >= (L/4)*G.  Needs L % 4 == 0 and K <= 24.  The features are bit-identical to mnr_cast_rays_ipe's rows; only the order
 * of the fp32 MFMA accumulation over layer 0's K differs from mnr_mlp_chain_fwd on that matrix. */
#define MNR_CHAIN_IPE_GROUP_COLS 192
typedef struct {
  mnr_ipe_cfg cfg;
  int n;                       /* samples per ray: row r of the level is sample r % n of ray r / n */
  const float* tdist;          /* [M/n, n+1] */
  const float* origins; const float* directions; const float* radii; const float* basis;   /* as mnr_cast_rays_ipe */
} mnr_chain_ipe_args;
int mnr_mlp_chain_fwd_ipe(const mnr_mlp_chain_fwd_args* chain, const mnr_chain_ipe_args* ipe, void* stream);

typedef struct {
  int64_t M; int W; int depth;
  const float* g_head;        /* [M] fp32: gradient w.r.t. the head output (from mnr_composite_bwd) */
  const float* w_head;        /* [W] fp32 head kernel */
  const uint8_t* bits[MNR_CHAIN_MAX_DEPTH];  /* ReLU masks written by the forward pass */
  const uint16_t* Bw[MNR_CHAIN_MAX_DEPTH];   /* layer i >= 1: [W, ldb[i]] bf16 = kernel as flax stores it (row = input) */
  int ldb[MNR_CHAIN_MAX_DEPTH];
  uint16_t* dY[MNR_CHAIN_MAX_DEPTH];         /* out: gradient w.r.t. layer i's pre-activation, [M, W] bf16
                                                (dY[depth-1] = mask * (g_head (x) w_head) may be NULL: not stored) */
  const uint16_t* dY_in;      /* optional: [M, W] bf16 gradient w.r.t. the LAST layer's pre-activation, already masked (an MLP
                                 with heads: the merged head's dX GEMM wrote it); then g_head / w_head / bits[depth-1] are unused
                                 and dY[depth-1] must be NULL */
} mnr_mlp_chain_bwd_args;
int mnr_mlp_chain_bwd(const mnr_mlp_chain_bwd_args* args, void* stream);

typedef struct {
  const uint16_t* A; int lda; int K;   /* A [M, lda] bf16, K columns used, K multiple of 128 */
  const uint16_t* B; int ldb; int N;   /* B [M, ldb] bf16, N columns used, N multiple of 128 */
  int64_t M;                           /* multiple of 64 */
  float* C; int ldc;                   /* fp32 [k_valid, ldc]: C[k,n] += sum_m A[m,k] B[m,n] */
  int k_valid, n_valid;                /* only k < k_valid, n < n_valid are written */
  float* bias_out; int bias_n_valid;   /* optional: bias_out[n] += sum_m B[m,n] for n < bias_n_valid
                                          (the Dense bias gradient, fused: B is read once) */
  const uint16_t* gcol; float* gcol_out;  /* optional (K, N multiples of 256): one more column of B given as a contiguous bf16
                                          vector [M] (32-byte aligned): gcol_out[k] += sum_m A[m,k] gcol[m] for k < k_valid.  The Dense(1) density head
                                          of the merged NeRF head (models.py:460 next to :527): its gradient column rides in
                                          the bottleneck's weight-gradient GEMM as one extra MFMA per k-step instead of
                                          widening N from 256 to 384 */
  int a_layout, b_layout;              /* MNR_LAYOUT_* of A and B (PANEL: lda == K resp. ldb == N of the whole matrix, K and N
                                          multiples of 256; the 256 x 256 output tile only) */
  /* Pairing with the dX GEMM that reads the same B (= dY) matrix (Model backward, one layer): m_interleave = 1 hands the
   * M-splits the 256-row M-tiles block-cyclically (split s takes M-tiles s, s + splits, ...) so that every split walks M from
   * top to bottom at the pace of a persistent NT launch running next to it; max_wgs > 0 caps the grid (the two launches then
   * share the chip).  Performance only: where M / 256 is not a multiple of the split count the launcher picks
   * (shape- and CU-count-dependent), m_interleave is dropped and the splits are contiguous. */
  int m_interleave, max_wgs;
  /* B given by its factors instead of as a matrix (then B may be NULL; row-major A, K and N multiples of 256):
   *   B[m, n] = bit n of rank1_bits[m, :] ? bf16(rank1_g[m] * rank1_w[n]) : 0
   * the gradient w.r.t. the LAST hidden layer's pre-activation of an MLP whose only head is Dense(1) (the proposal MLP,
   * models.py:460: dY_last = relu'(z_last) * (g_density (x) w_density)), value for value what mnr_mlp_chain_bwd computes and would
   * otherwise have to store for this launch to read back (M x N x 2 bytes each way).  rank1_g: fp32 [M] (4-byte aligned),
   * rank1_w: fp32 [N] (16-byte aligned), rank1_bits: the forward pass's 1-bit ReLU masks, row-major, bit (n & 7) of byte
   * [m * ld_rank1_bits + n / 8] (4-byte aligned, ld_rank1_bits a multiple of 4). */
  const float* rank1_g; const float* rank1_w; const uint8_t* rank1_bits; int ld_rank1_bits;
} mnr_gemm_tn_args;

/* Weight gradient: C += A^T B (fp32 atomics; C must be initialised by the caller). */
int mnr_gemm_tn_bf16(const mnr_gemm_tn_args* args, void* stream);

/* out[n] += sum_m X[m,n] for n < n_valid (bias gradient). X bf16 [M, ld]. */
int mnr_colsum_bf16(const uint16_t* X, int ld, int64_t M, int n_valid, float* out, void* stream);

/* One entry of the weight-packing table: copy an fp32 [rows_in, cols_out] flax
 * kernel (params + src_off) into a bf16 matrix at dst_off, as itself
 * (transpose=0: dst[r*ld + c]) or transposed (transpose=1: dst[c*ld + r]),
 * starting at (row0, col0) of the destination. */
typedef struct {
  int64_t src_off; int rows_in; int cols_out;
  int64_t dst_off; int ld; int row0; int col0; int transpose;
} mnr_pack_desc;
int mnr_pack_weights_bf16(const float* params, const mnr_pack_desc* descs_device, int n_desc,
                          int max_elems, uint16_t* dst, void* stream);

/* dst[k*ld_dst + c] (fp32, flat-gradient layout) += src[(row0+k)*ld_src + col0 + c] for
 * k < rows, c < cols: scatter a (padded / merged) weight-gradient block into
 * the flat gradient vector. */
int mnr_scatter_add_f32(const float* src, int ld_src, int row0, int col0, int rows, int cols,
                        float* dst, int ld_dst, void* stream);

/* fp32 -> bf16 cast of a strided matrix [M, n] (ld_src) into dst [M, ld_dst] at col0. */
int mnr_cast_f32_to_bf16(const float* src, int ld_src, int64_t M, int n, uint16_t* dst, int ld_dst,
                         int col0, void* stream);

/* Non-ReLU MLP.net_activation (models.py:348,457,578; jax.nn.softplus / jax.nn.silu are the ones the reference registers,
 * configs.py:29-31).  The Dense GEMM stores the bf16 pre-activation z [n elements, contiguous]:
 *   mnr_act_fwd_bf16: a = act(z);   mnr_act_bwd_bf16: d *= act'(z) in place (d = gradient w.r.t. a -> w.r.t. z).
 * kind: 1 = softplus, 2 = silu; arithmetic in fp32, one bf16 rounding. */
int mnr_act_fwd_bf16(int kind, int64_t n, const uint16_t* z, uint16_t* a, void* stream);
int mnr_act_bwd_bf16(int kind, int64_t n, const uint16_t* z, uint16_t* d, void* stream);
/* The same activations inside the forward-mode tangent network of the density-gradient normals (models.py:478-492: with a
 * non-ReLU net_activation jax differentiates through act' as well).  z [n = M*W] the layer's primal pre-activation, U [3n] its
 * tangent pre-activation (rows c*M + s = direction c of sample s):
 *   mnr_act_tangent_fwd_bf16: T[3n] = act'(z) * U;
 *   mnr_act_tangent_bwd_bf16: G[3n] (d loss / d T) becomes G * act'(z) in place, and extra[n] = sum_c G_c * U_c * act''(z) =
 *   d loss / d z through act', to be added to the primal backward pass's gradient of that layer. */
int mnr_act_tangent_fwd_bf16(int kind, int64_t n, const uint16_t* z, const uint16_t* U, uint16_t* T, void* stream);
int mnr_act_tangent_bwd_bf16(int kind, int64_t n, const uint16_t* z, const uint16_t* U, uint16_t* G, uint16_t* extra, void* stream);

/* X[m, c] += scale * noise[m, c] (fp32 add, one bf16 rounding) for the first `cols` columns of the bf16 matrix X [M, ld]:
 * the bottleneck noise of models.py:530-533 (`bottleneck += bottleneck_noise * random.normal(...)`) on the
 * bottleneck columns of the view-MLP input.  noise fp32 [M, cols], cols %% 8 == 0. */
int mnr_add_noise_bf16(int64_t M, int cols, uint16_t* X, int ld, const float* noise, float scale, void* stream);

/* Small-N dense VJP pieces (heads with 1..4 outputs, e.g. the rgb Dense(3)):
 *  dX[m,k] = relu'(H[m,k]) * sum_c g[m,c] W[k,c]          (bf16 out)
 *  dW[k,c] += sum_m H[m,k] g[m,c];  db[c] += sum_m g[m,c]  (fp32 atomics)
 * H bf16 [M, ldh] (K columns), g fp32 [M, C], W fp32 [K, C] (flax kernel). */
int mnr_small_head_bwd(int64_t M, int K, int C, const uint16_t* H, int ldh, const float* g,
                       const float* W, uint16_t* dX, int lddx, int apply_relu_mask,
                       float* dW, float* db,
                       const uint8_t* mask_bits /* optional 1-bit mask [*, ld_bits], row m %% bits_row_mod */,
                       int ld_bits, int64_t bits_row_mod,
                       float* scratch /* optional workspace for per-workgroup dW/db partials (else fp32 atomics) */,
                       int64_t scratch_floats, void* stream);

/* ------------------------------------------------------------------------- *
 * Compositing  (replaces the density/rgb activations models.py:506,584-602,
 * render.compute_alpha_weights render.py:130-151, render.volumetric_rendering
 * render.py:154-213 and stepfun.weighted_percentile stepfun.py:298-308)
 * ------------------------------------------------------------------------- */
typedef enum { MNR_ACT_SIGMOID = 0, MNR_ACT_SAFE_EXP = 1, MNR_ACT_SOFTPLUS = 2, MNR_ACT_EXP = 3,
               MNR_ACT_RELU = 4 } mnr_act;

typedef struct {
  int n;                   /* intervals per ray                                      */
  int opaque_background;   /* Model.opaque_background                                */
  int density_act;         /* mnr_act (softplus default)                             */
  float density_bias;      /* MLP.density_bias                                       */
  float density_noise_std; /* MLP.density_noise (0: none)                            */
  int has_rgb;             /* 0: MLP.disable_rgb (rgb = 0)                           */
  int rgb_act;             /* mnr_act                                                */
  float rgb_premultiplier, rgb_bias, rgb_padding;
  int bg_mode;             /* 0: scalar bg_value; 1: per-ray bg [B,3]                */
  float bg_value;
} mnr_composite_cfg;

/* raw_density [B,n] (Dense(1) output incl. its bias), density_noise [B,n] or
 * NULL, raw_rgb [B,n,3] or NULL, tdist [B,n+1], dirs [B,3], bg [B,3] or NULL,
 * exposure_scale [B,3] or NULL (RawNeRF models.py:257-267, already combined).
 * Outputs: density [B,n], rgb [B,n,3] (NULL if !has_rgb), weights [B,n],
 * rgb_out [B,3], acc [B]. */
int mnr_composite_fwd(const mnr_composite_cfg* cfg, int64_t B, const float* raw_density,
                      const float* density_noise, const float* raw_rgb, const float* tdist,
                      const float* dirs, const float* bg, const float* exposure_scale,
                      float* density, float* rgb, float* weights, float* rgb_out, float* acc,
                      void* stream);

/* VJP of mnr_composite_fwd.  g_rgb_out [B,3] or NULL, g_weights [B,n] or NULL
 * (from the interlevel / distortion losses).  Outputs: g_raw_density [B,n]
 * fp32 (and, if g_raw_density_bf16 != NULL, the same value as bf16 at
 * g_raw_density_bf16[row*ld_bf16], the density column of the head-gradient
 * matrix), g_raw_rgb [B,n,3] or NULL. */
int mnr_composite_bwd(const mnr_composite_cfg* cfg, int64_t B, const float* raw_density,
                      const float* density_noise, const float* raw_rgb, const float* tdist,
                      const float* dirs, const float* bg, const float* exposure_scale,
                      const float* weights, const float* g_rgb_out, const float* g_weights,
                      float* g_raw_density, uint16_t* g_raw_density_bf16, int ld_bf16,
                      float* g_raw_rgb, float* g_exposure_scale /* [B,3] +=, may be NULL */, void* stream);

/* One level's backward pass in one launch: the training losses acting on this level's rendering with their gradients
 * (train_utils.py:72-159: compute_data_loss on the composited colour; interlevel_loss of a proposal level against the
 * final level's histogram, stepfun.py:64-86; distortion_loss of the final level, stepfun.py:266-276) fused with the
 * compositing VJP (render.py:130-213).  d loss / d weights and d loss / d rgb never touch HBM.  Replaces one
 * mnr_data_loss + mnr_interlevel_loss | mnr_distortion_loss + mnr_composite_bwd sequence; mnr_composite_bwd is this
 * entry with both losses off. */
typedef struct {
  mnr_composite_cfg cfg;
  int64_t B, B_valid;           /* rays (padded), rays that take part in the losses */
  /* compositing VJP: as mnr_composite_bwd */
  const float* raw_density; const float* density_noise; const float* raw_rgb; const float* tdist; const float* dirs;
  const float* bg; const float* exposure_scale; const float* weights;
  const float* g_rgb_out;       /* optional upstream [B,3], added to the fused data-loss gradient */
  const float* g_weights;       /* optional upstream [B,n] (Ref-NeRF normal losses), added to the fused weight loss's */
  float* g_raw_density; uint16_t* g_raw_density_bf16; int ld_bf16; float* g_raw_rgb; float* g_exposure_scale;
  /* data loss; data_loss_type < 0: off.  data_stats[0] += weighted mse, [1] += data_loss_mult * loss (both / *denom) */
  int data_loss_type; float charb_padding; float data_loss_mult;
  const float* rgb_out; const float* gt; const float* lossmult; int lm_c; const float* denom; float* data_stats;
  /* loss on the weights: 0 none; 1 interlevel, this level = envelope of (t_ref [B,n_ref+1], w_ref [B,n_ref]);
   * 2 distortion on this level's own histogram.  sdist [B,n+1]: this level's normalised distances.  *wloss_stat += loss */
  int wloss_mode; float wloss_mult; const float* sdist; int n_ref; const float* t_ref; const float* w_ref; float* wloss_stat;
  /* optional output [B,n] fp32: d loss / d (sigma_i * delta_i), the optical-depth increments of render.py:144-145 -- what
   * Model.stop_level_grad = False needs to carry the compositing's gradient on to the sample distances (mnr_sdist_bwd) */
  float* g_x;
} mnr_level_bwd_args;
int mnr_level_bwd(const mnr_level_bwd_args* args, void* stream);

/* Model.stop_level_grad = False (models.py:56,198-201): d loss / d sdist [B,n+1] of one level, gathered per fence-post from
 *   g_x [B,n] (mnr_level_bwd: the optical-depth increments sigma_i * (t_{i+1} - t_i) * |d|, render.py:144-145; needs raw_density
 *     [B,n] with density_noise / density_noise_std / density_bias / density_act as in mnr_composite_cfg, and dirs [B,3]),
 *   g_t0, g_t1 [B*n] (mnr_cast_rays_ipe_bwd: the Gaussians' dependence on the interval ends, render.py:103-127),
 *     both through s_to_t' (coord.py:96-98; raydist_fn, near, far [B], sdist [B,n+1]),
 *   the distortion loss's own dependence on sdist (stepfun.py:266-276; distortion_mult != 0: weights [B,n], mean over B_valid rays),
 *   g_sdist_in [B,n+1]: what the NEXT level's resampling sends back (mnr_resample_level_bwd).
 * Every input group is optional (NULL / 0).  The interlevel loss is piecewise constant in sdist (stepfun.py:64-77). */
typedef struct {
  int64_t B, B_valid; int n;
  const float* sdist; const float* near; const float* far; int raydist_fn;
  const float* g_x; const float* raw_density; const float* density_noise; float density_noise_std; float density_bias;
  int density_act; const float* dirs;
  const float* g_t0; const float* g_t1;
  float distortion_mult; const float* weights;
  const float* g_sdist_in;
  float* g_sdist;
} mnr_sdist_bwd_args;
int mnr_sdist_bwd(const mnr_sdist_bwd_args* args, void* stream);

/* RawNeRF exposure (replaces models.py:257-267).  out[b,c] = exposure_values[b] *
 * (1 + [idx[b] > 0] * offsets[idx[b], c]); offsets = the 'exposure_scaling_offsets' embedding
 * [num_embeddings,3] or NULL when Model.learned_exposure_scaling is off.  The backward scatters
 * g_offsets[idx[b], c] += exposure_values[b] * g_scale[b, c] for idx[b] > 0. */
int mnr_exposure_scale(int64_t B, const float* exposure_values, const int32_t* exposure_idx,
                       const float* offsets, float* out, void* stream);
int mnr_exposure_scale_bwd(int64_t B_valid, const float* exposure_values, const int32_t* exposure_idx,
                           const float* g_scale, float* g_offsets, void* stream);

/* The compute_extras outputs of render.volumetric_rendering (render.py:184-211):
 * distance_mean, distance_percentile_5 / median / percentile_95 -> out [B,4]. */
int mnr_render_extras(int64_t B, int n, const float* weights, const float* tdist, const float* t_far,
                      float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Ref-NeRF branch  (replaces models.py:478-503,512-523,540-563,588-602, ref_utils.py:22-42,99-159,
 * image.py:48-56, train_utils.py:162-197).  Merged head column layout, bw = bottleneck width:
 *   [0,bw) bottleneck | bw density | bw+1..3 grad_pred | bw+4..6 raw diffuse | bw+7..9 raw tint | bw+10 raw roughness
 * `small` [M,11] fp32 = columns bw..bw+10 of the head GEMM; `raw_grad` [3,M] fp32 = d raw_density/d mean.
 * ------------------------------------------------------------------------- */
typedef struct {
  int T; int lmax;            /* number of (m,l) terms; largest degree (<= 16) */
  const int32_t* m; const int32_t* l;   /* [T] device arrays (ref_utils.get_ml_array) */
  const float* sigma;         /* [T] 0.5 l (l+1) */
  const float* mat;           /* [lmax+1, T] z-polynomial coefficients (ref_utils.py:119-125) */
} mnr_ide_tables;

/* Which parts of the branch an MLP has (models.py:468-563 takes every flag on its own; a head that is switched off is a zero
 * column of `small` nobody reads).  What the reference itself cannot run is refused with its own message where it has one:
 * reflections or n.v without a normal field (models.py:434-435), the IDE without the predicted roughness or on the per-ray
 * view direction (ref_utils.py:147-154: `kappa_inv` None / [B,36] against [B,n,1]). */
#define MNR_REF_PRED_NORMALS    1   /* enable_pred_normals: grad_pred columns, normals_to_use = normals_pred (:494-499) */
#define MNR_REF_DENSITY_NORMALS 2   /* disable_density_normals = False: raw_grad, normals (:478-492) */
#define MNR_REF_REFLECT         4   /* use_reflections (:540-547); else the view direction is encoded (:549-555) */
#define MNR_REF_IDE             8   /* use_directional_enc (:436-437); else coord.pos_enc(dir, 0, deg_view, True) (:438-441) */
#define MNR_REF_N_DOT_V        16   /* use_n_dot_v (:560-563) */
#define MNR_REF_ROUGHNESS      32   /* enable_pred_roughness (:520-523) */

/* normals = -l2norm(raw_grad), normals_pred = -l2norm(grad_pred), roughness = softplus(raw + bias),
 * dir = reflect(-viewdirs, normals_to_use) or viewdirs, IDE(dir, roughness) or pos_enc(dir) and n.v written (bf16) into
 * columns [col0, col0 + E (+ 1)) of every row of `vi` [M, ldvi], E = 2T or 3 + 6 deg_view; columns up to col_end
 * zero-filled.  Outputs (and `raw_grad`, `tabs`) of parts that are off may be NULL. */
int mnr_ref_head_fwd(int64_t M, int n, const float* small, const float* raw_grad, const float* viewdirs,
                     const mnr_ide_tables* tabs, int features, int deg_view, float roughness_bias, uint16_t* vi, int ldvi,
                     int col0, int col_end, float* normals_out, float* normals_pred_out, float* roughness_out, void* stream);
/* VJP: dvi_a (+ dvi_b, may be NULL) bf16 [M, lddvi] = gradient w.r.t. the view-MLP input; g_npred / g_n
 * [M,3] fp32 from mnr_ref_losses (may be NULL).  Writes bf16 columns [0,col0) (bottleneck = dvi_a + dvi_b),
 * col_gp..+2 (predicted normals) and col_rough (roughness) of dhb [M, lddhb] and g_raw_grad [3,M] fp32 (density normals).
 * col0 > 0 needs col0, lddvi and lddhb to be multiples of 8 (the bottleneck copy moves 16 bytes); a refused call writes nothing. */
int mnr_ref_head_bwd(int64_t M, int n, const float* small, const float* raw_grad, const float* viewdirs,
                     const mnr_ide_tables* tabs, int features, int deg_view, float roughness_bias, const uint16_t* dvi_a,
                     const uint16_t* dvi_b, int lddvi, int col0, const float* g_npred, const float* g_n,
                     uint16_t* dhb, int lddhb, int col_gp, int col_rough, float* g_raw_grad, void* stream);
/* dst[:, :cols] = a[:, :cols] + b[:, :cols] (bf16, b may be NULL; dst may alias a): gradient joins of skip concats. */
int mnr_add_cols_bf16(int64_t M, int cols, const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* dst,
                      int lddst, void* stream);
/* rgb = clip(linear_to_srgb(tint * sigmoid(premult raw_rgb + bias) + sigmoid(raw_diffuse - log 3)), 0, 1)
 * * (1 + 2 pad) - pad; VJP writes g_raw_rgb [M,3] fp32 and the diffuse / tint columns of dhb (bf16). */
int mnr_ref_color_fwd(int64_t M, const float* raw_rgb, const float* small, float rgb_premultiplier, float rgb_bias,
                      float rgb_padding, int use_tint, float* rgb_out, void* stream);
int mnr_ref_color_bwd(int64_t M, const float* raw_rgb, const float* small, float rgb_premultiplier, float rgb_bias,
                      float rgb_padding, int use_tint, const float* g_rgb, float* g_raw_rgb, uint16_t* dhb,
                      int lddhb, int col_diffuse, int col_tint, void* stream);
/* One level of orientation_loss + predicted_normal_loss: stats[0] += mult_o * mean_rays sum_i w min(0, n.(-v))^2,
 * stats[1] += mult_p * mean_rays sum_i w (1 - n.n_pred); g_weights [B,n] +=, g_normals / g_normals_pred [M,3] =. */
int mnr_ref_losses(int64_t B_valid, int n, float mult_orientation, float mult_pred_normal, int target_is_pred,
                   const float* weights, const float* normals, const float* normals_pred, const float* viewdirs,
                   float* stats, float* g_weights, float* g_normals, float* g_normals_pred, void* stream);
/* out[b,c] = sum_i weights[b,i] values[b,i,c]  (render.py:187-190 extras). */
/* Predicted normals without the rest of the Ref-NeRF head (internal/models.py:494-503 with enable_pred_normals only):
 * normals_pred[M,3] = -l2_normalize(small[:, col .. col+2]) (ref_utils.py:40-42) from the head GEMM's fp32 side output [M, ld];
 * _bwd: the VJP of the same into columns col_g .. col_g+2 of the head's bf16 gradient matrix [M, lddhb].
 * mnr_ref_losses takes normals = NULL for such an MLP (mult_pred_normal == 0, target_is_pred = 1, g_normals = NULL). */
/* Density-gradient normals without the rest of the Ref-NeRF head (internal/models.py:478-492 with disable_density_normals = False
 * only): normals[M,3] = -l2_normalize(raw_grad) from the tangent network's raw_grad [3, M] (component-major); _bwd: g_raw_grad [3, M].
 * mnr_ref_losses takes normals_pred = NULL for such an MLP (mult_pred_normal == 0, target_is_pred = 0, g_normals_pred = NULL). */
int mnr_density_normals_fwd(int64_t M, const float* raw_grad, float* normals_out, void* stream);
int mnr_density_normals_bwd(int64_t M, const float* raw_grad, const float* g_normals, float* g_raw_grad, void* stream);
int mnr_pred_normals_fwd(int64_t M, const float* small, int ld, int col, float* normals_pred_out, void* stream);
int mnr_pred_normals_bwd(int64_t M, const float* small, int ld, int col, const float* g_normals_pred, uint16_t* dhb, int lddhb,
                         int col_g, void* stream);
int mnr_weighted_sum(int64_t B, int n, int C, const float* weights, const float* values, float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Losses  (replaces train_utils.compute_data_loss train_utils.py:72-136,
 * interlevel_loss :139-150 with stepfun.lossfun_outer stepfun.py:30-86,
 * distortion_loss :153-159 with stepfun.lossfun_distortion stepfun.py:266-276)
 * Scalars accumulate into `stats` (fp32 device array, zeroed by the caller).
 * ------------------------------------------------------------------------- */
typedef enum { MNR_LOSS_MSE = 0, MNR_LOSS_CHARB = 1, MNR_LOSS_RAWNERF = 2 } mnr_data_loss_type;

/* out[0] += sum(lossmult broadcast to [B,3]) over the first B_valid rays. lossmult [B,lm_c], lm_c in {1,3}. */
int mnr_lossmult_sum(int64_t B_valid, const float* lossmult, int lm_c, float* out, void* stream);

/* compute_data_loss's gradient-free metrics (train_utils.py:113-128), either may be NULL:
 * *out_disp = mean (1/(1+distance_mean) - disps)^2;  *out_normal = weighted mean angular error in degrees
 * (ref_utils.compute_weighted_mae ref_utils.py:45-50) with weights acc * alphas. */
int mnr_render_metrics(int64_t B_valid, const float* distance_mean, const float* disps, const float* acc,
                       const float* alphas, const float* normals, const float* normals_gt, float* out_disp,
                       float* out_normal, void* stream);

/* One level of compute_data_loss.  rgb [B,3] rendered, gt [B,3], denom = device
 * scalar from mnr_lossmult_sum.  stats[0] += mse numerator/denom, stats[1] +=
 * loss_mult * data loss.  g_rgb [B,3] (may be NULL) = d(loss_mult*loss)/d rgb. */
int mnr_data_loss(int loss_type, float charb_padding, float loss_mult, int64_t B, int64_t B_valid,
                  const float* rgb, const float* gt, const float* lossmult, int lm_c,
                  const float* denom, float* stats, float* g_rgb, void* stream);

/* interlevel: t [B,n+1], w [B,n] (final level, constants); t_env [B,ne+1], w_env
 * [B,ne] (proposal).  stats[0] += mult * mean(lossfun_outer); g_w_env [B,ne]
 * (+=, may be NULL) = d/d w_env. */
int mnr_interlevel_loss(float mult, int64_t B, int64_t B_valid, int n, const float* t, const float* w,
                        int ne, const float* t_env, const float* w_env, float* stats, float* g_w_env,
                        void* stream);

/* distortion on (t = sdist, w): stats[0] += mult * mean(lossfun_distortion); g_w [B,n] += d/d w. */
int mnr_distortion_loss(float mult, int64_t B, int64_t B_valid, int n, const float* t, const float* w,
                        float* stats, float* g_w, void* stream);

/* Leaf for parity: per-ray lossfun_outer [B,n] and lossfun_distortion [B]. */
int mnr_lossfun_outer(int64_t B, int n, const float* t, const float* w, int ne, const float* t_env,
                      const float* w_env, float* out, void* stream);
int mnr_lossfun_distortion(int64_t B, int n, const float* t, const float* w, float* out, void* stream);

/* RobustNeRF (Config.data_loss_type = 'robustnerf'): the binary inlier mask of robustnerf.py:23-86 for one level's
 * rendering.  The first B_valid rays are num_patches * P * P pixels in [patch][y][x] order, one workgroup per patch.
 * A pixel is kept when its error mean_c (rgb - gt)^2 lies below *loss_threshold, or when more than
 * 1 - smoothed_inlier_quantile of its f x f neighbourhood does ('SAME' zero padding, always over f * f), or when it lies
 * in the centred inner x inner square of a patch of which more than 1 - inner_patch_inlier_quantile of the pixels pass
 * one of the first two tests.  Votes are counted in integers and compared as count / n in double.  enable = 0: the
 * mask is all ones (robustnerf.py:29-33) and only stats[3] is produced.  Limits: P * P <= 1024, f odd and <= P,
 * inner <= P, B_valid a multiple of P * P.  Nothing is read back: the threshold and the results stay on the device. */
typedef struct {
  int64_t B, B_valid;              /* rays (padded), rays that take part */
  int patch_size, inner_patch_size, filter_size, enable;
  double smoothed_inlier_quantile, inner_patch_inlier_quantile;
  const float* rgb;                /* [B,3] rendered */
  const float* gt;                 /* [B,3] */
  const float* lossmult;           /* [B,lm_c] */
  int lm_c;                        /* 1 or 3 */
  const float* loss_threshold;     /* device scalar */
  const float* denom;              /* device scalar (mnr_lossmult_sum); read only when mse is given */
  float* mask;                     /* [B]: 1 inlier, 0 outlier, 0 for the padding rays */
  float* lossmult_out;             /* [B,lm_c] = lossmult * mask, may be NULL */
  float* err;                      /* [B]: per-pixel error mean_c (rgb - gt)^2 of the first B_valid rays (mnr_quantile's input), may be NULL */
  float* stats;                    /* [4] += mean is_inlier_loss, has_inlier_neighbors, is_inlier_patch, mask; may be NULL */
  float* mse;                      /* [1] += sum(lossmult * (rgb - gt)^2) / *denom with the UNMASKED lossmult
                                      (train_utils.py:86-88); may be NULL */
} mnr_robust_args;
int mnr_robustnerf_mask(const mnr_robust_args* args, void* stream);

/* jnp.quantile(x[0:N], q), linear interpolation between the two exact order statistics at floor and ceil of
 * q * (M - 1) over the M finite values of x (non-finite values are ignored; *out = NaN when there is none).  Exact
 * selection (radix select on the bit patterns) in one workgroup, deterministic, any N >= 1, 0 <= q <= 1. */
int mnr_quantile(int64_t N, const float* x, double q, float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Optimiser  (replaces train_utils.clip_gradients train_utils.py:200-218,
 * jnp.nan_to_num :328 and optax.adam state.apply_gradients :330,372)
 * ------------------------------------------------------------------------- */
/* Weight regulariser of one top-level module (train_utils.py:300-305, Config.weight_decay_mults):
 * *loss_out += mult * sum(params[begin:end]^2); grad[begin:end] += 2 mult params; *sqnorm_out += sum p^2
 * (stats['weight_l2s']).  grad / loss_out / sqnorm_out may be NULL. */
int mnr_weight_decay(const float* params, int64_t begin, int64_t end, float mult, float* grad, float* loss_out,
                     float* sqnorm_out, void* stream);

/* out[0] += sum of squares of grad[begin:end] (each element first clipped to
 * +-max_val when max_val > 0): one call per top-level module. */
int mnr_grad_sqnorm(const float* grad, int64_t begin, int64_t end, float max_val, float* out, void* stream);

typedef struct {
  float lr, b1, b2, eps;
  float bias_corr1, bias_corr2;  /* 1 - b1^t, 1 - b2^t                          */
  float one_minus_b1, one_minus_b2; /* float(1 - b) formed in double, as optax does: 1.0f - 0.999f is 0.00099998713f, not 0.001f */
  float grad_max_val;            /* 0: off                                      */
  float grad_max_norm;           /* 0: off                                      */
} mnr_adam_cfg;

/* For one segment [begin,end): g = clip_value(g); g *= min(1, max_norm/(eps32+sqrt(sqnorm[seg])));
 * g = nan_to_num(g); Adam moments and parameter update in place. */
int mnr_clip_adam(const mnr_adam_cfg* cfg, int64_t begin, int64_t end, const float* sqnorm_seg,
                  const float* grad, float* params, float* mu, float* nu, void* stream);

/* ------------------------------------------------------------------------- *
 * Evaluation metrics  (replaces internal/image.py: MetricHarness :127-141 with dm_pix.ssim, color_correct :81-124, and
 * the quantise / crop / mean of eval.py:134-146).  Every sum is per-workgroup partials in float64 added by a second,
 * fixed-order stage: no floating-point atomics, two runs agree bit for bit.  Results are device scalars in float64.
 * ------------------------------------------------------------------------- */
#define MNR_SSIM_MAX_FILTER 11

/* dm_pix.ssim(a, b) of two [H,W,C] float32 images: Gaussian window of `filter_size` taps (odd, <= MNR_SSIM_MAX_FILTER)
 * and `filter_sigma`, normalised to sum 1, applied separably per channel with VALID padding;
 * mu0, mu1 the windowed means, sigma00 = filt(a a) - mu0^2 and sigma11 likewise, both clamped at float32_eps^2,
 * sigma01 = filt(a b) - mu0 mu1 limited in magnitude to sqrt(sigma00 sigma11); c1 = (k1 max_val)^2, c2 = (k2 max_val)^2;
 * ssim_map = (2 mu0 mu1 + c1)(2 sigma01 + c2) / ((mu0^2 + mu1^2 + c1)(sigma00 + sigma11 + c2)); *out = its mean.
 * crop = c > 0 evaluates x[c:-c, c:-c] by index arithmetic.  One workgroup per 32 x 16 output tile and channel; window
 * sums in float64.  `map` (may be NULL) receives ssim_map as [H - 2c - f + 1, W - 2c - f + 1, C] float32. */
typedef struct {
  int H, W, C, crop;
  int filter_size;
  double filter_sigma, max_val, k1, k2;
  const float* a;
  const float* b;
  float* map;
  double* partials;                /* workspace of mnr_ssim_partials(...) doubles */
  double* out;                     /* [1] */
} mnr_ssim_args;
int mnr_ssim_partials(int H, int W, int C, int crop, int filter_size);    /* <= 0: the arguments are not valid */
int mnr_ssim(const mnr_ssim_args* args, void* stream);

/* out[0] = sum (q(a) - b)^2 over x[c:-c, c:-c] of two [H,W,C] images, in float64; quantize != 0: q(a) = rint(255 a) / 255
 * (round half to even, np.round), else q(a) = a.  a / b are float64 when a_f64 / b_f64 is set, else float32.  q_out
 * (may be NULL) receives q(a) of the WHOLE image as float32 (what mnr_ssim takes).  partials: workspace of
 * mnr_image_sqdiff_partials(H * W * C) doubles. */
typedef struct {
  int H, W, C, crop, quantize, a_f64, b_f64;
  const void* a;
  const void* b;
  float* q_out;
  double* partials;
  double* out;                     /* [1] */
} mnr_sqdiff_args;
int mnr_image_sqdiff_partials(int64_t n);
int mnr_image_sqdiff(const mnr_sqdiff_args* args, void* stream);

/* One iteration of image.color_correct (internal/image.py:95-122), left-hand side.  Per pixel the ten features
 * r r, r g, r b, g g, g b, b b, r, g, b, 1 of img [N,3] (float64); per channel c, over the rows where
 * mask0[:, c] & unclipped(img[:, c]) & unclipped(ref[:, c]) holds (unclipped(z): eps <= z <= 1 - eps), the symmetric
 * A^T A and A^T b with b = ref[:, c].  out [3][65] float64: the 55 entries i <= j of A^T A in row-major order of the
 * upper triangle, then the 10 of A^T b.  write_mask0 != 0: mask0 = unclipped(img) is WRITTEN (the first iteration,
 * image.py:91) instead of read.  partials: workspace of mnr_cc_gram_partials(N) doubles. */
#define MNR_CC_FEATURES 10
#define MNR_CC_GRAM_OUT 65
typedef struct {
  int64_t N;
  double eps;
  const double* img;               /* [N,3] current corrected image */
  const double* ref;               /* [N,3] */
  unsigned char* mask0;            /* [N,3] */
  int write_mask0;
  double* partials;
  double* out;                     /* [3][MNR_CC_GRAM_OUT] */
} mnr_cc_gram_args;
int mnr_cc_gram_partials(int64_t N);
int mnr_cc_gram(const mnr_cc_gram_args* args, void* stream);

/* out[i, c] = clip(sum_k feature_k(img[i]) warp[k][c], 0, 1) in float64 (image.py:121-122); out may alias img. */
int mnr_cc_apply(int64_t N, const double* img, const double* warp /* host [10][3] */, double* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Visualisation  (the per-pixel work of internal/vis.py and of render.py:86-93; csrc/vis.hip)
 * float32 device images in, float64 arithmetic, one rounding at the store.
 * ------------------------------------------------------------------------- */
#define MNR_VIS_MAX_PERCENTILES 4

/* vis.weighted_percentile(x, w, ps) (vis.py:22-30) on ordered data: x_sorted [N] ascending, order [N] (int64) the index
 * every sorted value had before the sort, w [NW] the weights as given.  The weight of sorted element i is
 * w[min(order[i], NW - 1)] (jax clamps an out-of-range gather index; visualize_suite's depth triplet has N = 3 NW).
 * acc = running sum of those weights in float64, T = p acc[-1] / 100, out[k] = np.interp(T, acc, x_sorted): x[0] if
 * T < acc[0], x[-1] if T >= acc[-1], else with j the LAST index that has acc[j] <= T,
 * x[j] + (T - acc[j]) / (acc[j+1] - acc[j]) (x[j+1] - x[j]).  ps: HOST array of num_p <= 4 percentiles in [0, 100].
 * out [num_p] fp32 device.  partials: mnr_weighted_percentile_partials(N) doubles of device workspace.  Fixed-order sums,
 * no floating-point atomics: deterministic.  Any N >= 1; weights >= 0. */
int mnr_weighted_percentile_partials(int64_t N);
int mnr_weighted_percentile(int64_t N, const float* x_sorted, const int64_t* order, int64_t NW, const float* w, int num_p,
                            const double* ps, double* partials, float* out, void* stream);

/* x; log(x + eps32) and -log(x + eps32) (vis.visualize_suite's depth curves); log(x) (Config.render_dist_curve_fn) */
typedef enum { MNR_VIS_CURVE_IDENTITY = 0, MNR_VIS_CURVE_LOG = 1, MNR_VIS_CURVE_NEG_LOG = 2, MNR_VIS_CURVE_LN = 3 } mnr_vis_curve;

/* The per-pixel part of vis.visualize_cmap (vis.py:85-106): curve value, lo and hi; v = nan_to_num(clip((value -
 * min(lo, hi)) / |hi - lo|, 0, 1)), or mod(value, modulus) / modulus when modulus > 0; with a LUT (C = 1) the colour is
 * lut[min(trunc(v n_lut), n_lut - 1)], without (C = 3) the three normalised channels; with acc the result is matted over
 * the checker as mnr_vis_matte does.  out_u8 = trunc(clip(nan_to_num(colour), 0, 1) 255) (render.py:93). */
typedef struct {
  int H, W, C;
  const float* value;              /* [H,W,C] */
  const float* lohi;               /* device [2]: lo, hi BEFORE the curve; may be NULL when modulus > 0 */
  int curve;                       /* mnr_vis_curve */
  double modulus;                  /* <= 0: none */
  const float* lut;                /* [n_lut,3] or NULL */
  int n_lut;
  const float* acc;                /* [H,W] or NULL: no matte */
  float dark, light;
  int width;
  float* out;                      /* [H,W,3], may be NULL when out_u8 is given */
  unsigned char* out_u8;           /* [H,W,3] or NULL */
} mnr_vis_cmap_args;
int mnr_vis_cmap(const mnr_vis_cmap_args* args, void* stream);

/* vis.matte (vis.py:39-45): out = pre(x) acc + bg (1 - acc), bg = light where (row % 2w) / w xor (col % 2w) / w, else dark.
 * pre: x; x / 2 + 0.5 (normals); tanh(x) (roughness); ((origins + directions distance + 1) mod 2) / 2
 * (visualize_coord_mod, vis.py:109-111,185; C = 3, x unused; directions and distance may both be NULL: origins are the
 * coordinates). */
typedef enum { MNR_VIS_PRE_NONE = 0, MNR_VIS_PRE_HALF = 1, MNR_VIS_PRE_TANH = 2, MNR_VIS_PRE_COORD_MOD = 3 } mnr_vis_preop;
typedef struct {
  int H, W, C;
  int preop;                       /* mnr_vis_preop */
  const float* x;                  /* [H,W,C] */
  const float* acc;                /* [H,W] */
  const float* origins;            /* [H,W,3], MNR_VIS_PRE_COORD_MOD only */
  const float* directions;         /* [H,W,3] */
  const float* distance;           /* [H,W] */
  float dark, light;
  int width;
  float* out;                      /* [H,W,C] */
} mnr_vis_matte_args;
int mnr_vis_matte(const mnr_vis_matte_args* args, void* stream);

/* ------------------------------------------------------------------------- *
 * RawNeRF data path  (the per-pixel work of internal/raw_utils.py; csrc/raw.hip)
 * Deterministic: float64 sums are per-workgroup partials added in a fixed order, counts are integer atomics.
 * ------------------------------------------------------------------------- */
typedef enum { MNR_RAW_U16 = 0, MNR_RAW_F32 = 1 } mnr_raw_dtype;

/* raw_utils.load_raw_dataset:354-382 for a stack of Bayer mosaics [N,H,W] (RGGB, red at (0,0); H, W even; dtype a
 * mnr_raw_dtype): v = (raw - black[i]) / (white[i] - black[i]) * scale in float64, rounded once to float32 (black, white:
 * DEVICE [N] float64, both NULL: v = raw); raw_utils.bilinear_demosaic in float32, with the wrap-around of its np.roll at
 * the borders; n_downsample > 1 (must divide H and W): the area mean over n x n blocks (image.downsample), added in
 * float64 row by row and rounded once; the full-resolution image is not written.  out [N, H/n, W/n, 3] float32. */
int mnr_raw_demosaic(int N, int H, int W, int dtype, const void* mosaic, const double* black, const double* white,
                     double scale, int n_downsample, float* out, void* stream);

/* raw_utils.postprocess_raw in float64: rgb_lin = raw camtorgb^T; linear_only != 0: out_f64 = rgb_lin and nothing else
 * (what the exposure percentile is taken of).  Otherwise srgb = image.linear_to_srgb(clip(rgb_lin / exposure, 0, 1)), with
 * exposure = *exposure_dev when that is given (a device scalar: an auto-exposure needs no host read), else `exposure`.
 * Any subset of the outputs: out_f64, out_f32 (rounded once), out_u8 = trunc(clip(nan_to_num(srgb), 0, 1) 255)
 * (utils.save_img_u8). */
typedef struct {
  int64_t P;
  const void* raw;                 /* [P,3] float32, or float64 when raw_f64 is set */
  int raw_f64;
  double camtorgb[9];              /* row-major [3,3] */
  double exposure;
  const double* exposure_dev;      /* device [1] or NULL */
  int linear_only;
  double* out_f64;                 /* [P,3] or NULL */
  float* out_f32;                  /* [P,3] or NULL */
  unsigned char* out_u8;           /* [P,3] or NULL */
} mnr_raw_post_args;
int mnr_raw_postprocess(const mnr_raw_post_args* args, void* stream);

/* np.percentile(x[0:N], p) of float64 values, 0 <= p <= 100: the exact order statistics a, b at floor and ceil of
 * p / 100 (M - 1) over the M finite values (non-finite ones are ignored; *out = NaN when there is none), combined as numpy's
 * _lerp does: a + (b - a) t, or b - (b - a)(1 - t) for t >= 0.5.  Radix select on the 64-bit patterns, 8 bits a pass, over
 * many workgroups: per-workgroup LDS histograms merged by integer atomics.  workspace: mnr_quantile_f64_workspace(N)
 * bytes of device memory (0: N is not valid), overwritten.  out: device [1]. */
int64_t mnr_quantile_f64_workspace(int64_t N);
int mnr_quantile_f64(int64_t N, const double* x, double p, void* workspace, double* out, void* stream);

/* raw_utils.best_fit_affine's sums for axis = (0, 1): from est, gt [P,3] float64, out [4][3] float64 = per channel the sums
 * of gt, est, gt est, gt gt.  partials: workspace of mnr_affine_sums_partials(P) doubles. */
int mnr_affine_sums_partials(int64_t P);
int mnr_affine_sums(int64_t P, const double* est, const double* gt, double* partials, double* out, void* stream);

/* raw_utils.match_images_affine's last line: out[i, c] = (est[i, c] - b[c]) / a[c]; a, b: HOST [3]; out may alias est. */
int mnr_affine_apply(int64_t P, const double* est, const double* a, const double* b, double* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Image ingest  (what the dataset loaders do with decoded pixels; csrc/ingest.hip)
 * ------------------------------------------------------------------------- */
typedef enum { MNR_IMG_U8 = 0, MNR_IMG_F32 = 1 } mnr_img_dtype;
typedef enum { MNR_INGEST_PLAIN = 0, MNR_INGEST_WHITE_BG = 1, MNR_INGEST_NORMALS = 2 } mnr_ingest_mode;

/* src: DEVICE [N,H,W,C], 1 <= C <= 4, uint8 or float32 (dtype a mnr_img_dtype).  With n = n_downsample (must divide H and W),
 * h = H / n, w = W / n, per output pixel and channel the block mean m (image.downsample): uint8: the exact integer sum S
 * of the n x n block, m = float(S) / float(n n), one float32 division (n <= 256, so that S is exact); float32: the block
 * added in float64 row by row (dy outer, dx inner), divided by n n in float64 and rounded once.  n = 1: m is the value.
 * Then, every step rounded to float32 on its own (no fused multiply-add):
 *   MNR_INGEST_PLAIN     out [N,h,w,C_out] = the first C_out <= C channels of v, v = m / 255.f (uint8) or m (float32);
 *   MNR_INGEST_WHITE_BG  (C == 4, C_out == 3) out[c] = v[c] * v[3] + (1.f - v[3]); alpha [N,h,w], when not NULL, = v[3];
 *   MNR_INGEST_NORMALS   (uint8, C >= 3, C_out == 3) out[c] = m[c] * 2.f / 255.f - 1.f.
 * alpha must be NULL in the other modes.  n * C may not exceed 4096 (only a float32 input can get there).  N == 0 is a
 * successful no-op.  Invalid arguments return MNR_ERR_INVALID_ARGUMENT before anything is launched.  64-bit offsets; no
 * atomics: two runs agree bit for bit. */
int mnr_image_ingest(int N, int H, int W, int C, int dtype, const void* src, int n_downsample, int mode, int C_out,
                     float* out, float* alpha, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh extraction: marching tetrahedra on a regular grid  (csrc/mesh.hip)
 * field [nx,ny,nz] float32, every dimension >= 2, field[i,j,k] at origin + spacing (i,j,k); linear point index
 * p = (i ny + j) nz + k; a point is inside iff field >= level (a NaN is outside).  Every cell is cut into the 6 Kuhn
 * tetrahedra, one per permutation (a, b, c) of the axes in lexicographic order (corners p, p + e_a, p + e_a + e_b,
 * p + (1,1,1)); an edge leaves its lower end in one of the 7 directions (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1),
 * (0,1,1), (1,1,1) and carries a vertex iff its ends differ.  Vertices are ordered by lower-end index, then direction:
 * the id of edge (p, e) is base[p] + popcount(mask[p] & ((1 << e) - 1)).  A vertex is P0 + t (P1 - P0) with
 * t = (level - f0) / (f1 - f0) (0.5 where that is outside [0, 1] or NaN) and P = origin + spacing float(index), float32,
 * no contraction; its normal is -g / |g| (0 where |g| is 0 or not finite) of the field gradient (central differences,
 * one-sided at the grid faces, over the spacing) interpolated with the same t.  Faces are ordered by cell index, then
 * tetrahedron, then triangle, counter-clockwise seen from the low-field side.  No atomics: two runs agree bit for bit.
 *
 * A workgroup owns 256 consecutive linear indices; mnr_mt_workgroups(n_points) is their number.  The caller runs
 * mnr_mt_classify (mask, counts), takes the exclusive scan of counts over the workgroups as int64 (offsets) and the totals
 * (n_verts, n_faces, both below 2^31), then mnr_mt_emit_vertices (base, verts, normals) and mnr_mt_emit_faces (faces).
 * The emit passes tolerate a mask or offsets that are not this field's (a stale workspace): mask bits of edges that leave the
 * grid are ignored, and nothing is written at or beyond row n_verts of verts / normals or row n_faces of faces; what is written
 * is then meaningless, but no access leaves the grid or the outputs.
 * ------------------------------------------------------------------------- */
typedef struct {
  int nx, ny, nz;
  const float* field;              /* [nx,ny,nz] */
  float level;
  float origin[3];
  float spacing;                   /* > 0, finite */
  unsigned char* mask;             /* [points]: written by classify, read by the emit passes */
  int* counts;                     /* [workgroups,2]: (vertices, triangles) per workgroup, written by classify */
  const int64_t* offsets;          /* [workgroups,2]: exclusive scan of counts (emit passes) */
  int* base;                       /* [points]: written by emit_vertices, read by emit_faces */
  float* verts;                    /* [n_verts,3] */
  float* normals;                  /* [n_verts,3] */
  int64_t n_verts;
  int* faces;                      /* [n_faces,3] */
  int64_t n_faces;
} mnr_mt_args;
int64_t mnr_mt_workgroups(int64_t n_points);
int mnr_mt_classify(const mnr_mt_args* args, void* stream);
int mnr_mt_emit_vertices(const mnr_mt_args* args, void* stream);
int mnr_mt_emit_faces(const mnr_mt_args* args, void* stream);

/* ------------------------------------------------------------------------- *
 * TSDF fusion of depth images into a regular grid, and vertex validity  (csrc/tsdf.hip)
 * The grid is the one above: voxel (i,j,k) at origin + spacing (i,j,k), linear index p = (i ny + j) nz + k.  proj [F,3,4] maps
 * world coordinates to (u zc, v zc, zc), pixel px covering [px, px + 1) and depth [F,H,W] holding zc of the surface (0, a
 * negative value, an infinity or a NaN: no measurement).  Per voxel, frames f = 0 .. F - 1 in ascending order, float32 in the
 * order written, no contraction:
 *   1. x = origin[0] + spacing float(i), likewise y, z;
 *   2. m_r = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3] for r = 0, 1, 2; zc = m_2; skip the frame unless zc > 0;
 *   3. u = m_0 / zc, v = m_1 / zc; skip unless 0 <= u < float(W) and 0 <= v < float(H); px = int(u), py = int(v);
 *   4. if acc is given and acc[f,py,px] < acc_threshold the ray is empty: t = 1;
 *   5. otherwise d = depth[f,py,px]; skip unless 0 < d < inf; s = d - zc; skip if s < -trunc; t = min(1, s / trunc);
 *   6. sum_t += t, sum_w += 1, sum_c[c] += rgb[f,py,px,c];
 *   7. after the last frame, if sum_w > 0: W0 = weight[p], Wn = W0 + sum_w, tsdf[p] = (W0 tsdf[p] + sum_t) / Wn,
 *      color[p,c] = (W0 color[p,c] + sum_c[c]) / Wn, weight[p] = Wn; otherwise the voxel is not written.
 * A launch stages at most MNR_TSDF_MAX_FRAMES matrices; a longer stack is integrated MNR_TSDF_MAX_FRAMES frames a launch, in
 * order, each launch applying step 7 to its own sums (so F = 100 equals a call with the first 64 frames followed by a call
 * with the other 36).  Within a launch every volume is read and written once.  F == 0 is a successful no-op.  No atomics: two
 * runs agree bit for bit.
 * ------------------------------------------------------------------------- */
#define MNR_TSDF_MAX_FRAMES 64
typedef struct {
  int nx, ny, nz;
  float origin[3];
  float spacing;                   /* > 0, finite */
  float trunc;                     /* world units, > 0, finite */
  int F, H, W;
  const float* proj;               /* [F,3,4] */
  const float* depth;              /* [F,H,W] */
  const float* acc;                /* [F,H,W] or NULL */
  float acc_threshold;
  const float* rgb;                /* [F,H,W,3] or NULL */
  float* tsdf;                     /* [nx,ny,nz], updated in place */
  float* weight;                   /* [nx,ny,nz], updated in place */
  float* color;                    /* [nx,ny,nz,3] or NULL (rgb and color: both or neither), updated in place */
} mnr_tsdf_args;
int mnr_tsdf_integrate(const mnr_tsdf_args* args, void* stream);

/* The same fusion for any camera model: cameras [F,MNR_CAM_REC] (device) holds one record a frame (the forward camera model
 * above), all of the model `model` and of the images' H and W; depth holds s, the distance rendered along the camera's own rays.
 * The seven steps stay, with steps 2 and 3 replaced by the forward model:
 *   2/3. (u, v, s, ok) of the frame's record at (x, y, z); skip the frame unless ok and 0 <= u < float(W) and 0 <= v < float(H);
 *        px = int(u), py = int(v);
 *   5.   ... skip unless 0 < d < inf; e = d - s; skip if e < -trunc; t = min(1, e / trunc).
 * A record whose model, H or W is not the call's is skipped as a whole.  Everything else (frames in ascending order, the sums
 * folded after the last frame of a launch, MNR_TSDF_MAX_FRAMES frames a launch, no atomics) is as stated above.  For
 * MNR_CAM_PERSPECTIVE a NumPy float32 restatement reproduces the volumes bit for bit; fisheye and pano call atan2f and acosf.
 * mnr_tsdf_integrate itself is untouched: an undistorted pinhole keeps its [3,4] matrix and its kernel. */
typedef struct {
  int nx, ny, nz;
  float origin[3];
  float spacing;                   /* > 0, finite */
  float trunc;                     /* world units, > 0, finite */
  int F, H, W;
  int model;                       /* mnr_camtype of every record */
  const float* cameras;            /* [F,MNR_CAM_REC] */
  const float* depth;              /* [F,H,W] */
  const float* acc;                /* [F,H,W] or NULL */
  float acc_threshold;
  const float* rgb;                /* [F,H,W,3] or NULL */
  float* tsdf;                     /* [nx,ny,nz], updated in place */
  float* weight;                   /* [nx,ny,nz], updated in place */
  float* color;                    /* [nx,ny,nz,3] or NULL (rgb and color: both or neither), updated in place */
} mnr_tsdf_cam_args;
int mnr_tsdf_integrate_cam(const mnr_tsdf_cam_args* args, void* stream);

/* keep[id] = 1 iff both ends of vertex id's grid edge have valid != 0, else 0, for the vertices of a mesh the three passes above
 * produced: args carries that run's nx, ny, nz, mask, base and n_verts; valid [points] and keep [n_verts] are bytes.  As in the
 * emit passes, mask bits of edges that leave the grid are ignored and nothing is written at or beyond keep[n_verts]. */
int mnr_mt_vertex_valid(const mnr_mt_args* args, const unsigned char* valid, unsigned char* keep, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh clean-up: connected components  (csrc/meshclean.hip)
 * faces [n_faces,3] int32 over vertices 0 .. n_verts - 1.  labels [n_verts] int32 converges to: labels[v] = the smallest vertex
 * id that v is connected to through face edges; a vertex in no face keeps its own id.  That result is unique, integer only
 * (atomicMin, no floating point), so two runs agree bit for bit however the atomics interleave.
 *   mnr_mesh_cc_init   labels[v] = v.
 *   mnr_mesh_cc_sweep  one round of hooking (per face: the smallest of its three labels m is min-ed into every vertex x of the
 *                      face whose label l is above m, and into labels[l]) and pointer jumping (per vertex: follow
 *                      l = labels[l] while it decreases, store the end).  Adds nothing to *changed (an int on the device) when
 *                      the hooking found every face with one label, stores 1 to it otherwise; it never stores 0.
 * The caller zeroes a flag, runs sweeps and reads the flag back: the sweep that leaves its flag 0 has changed nothing and
 * labels is the result (ops.mesh_components gives each sweep of a batch its own flag and reads a batch back at once).  A
 * fixed iteration count is not a stopping rule: a label may have to travel the diameter of the mesh.  An index in faces
 * outside [0, n_verts) makes its face be skipped, and every label is checked against [0, n_verts) before it is used as an
 * index: no access leaves labels whatever faces and labels hold.  n_verts == 0 or n_faces == 0: nothing is launched by a sweep.
 * ------------------------------------------------------------------------- */
int mnr_mesh_cc_init(int64_t n_verts, int* labels, void* stream);
int mnr_mesh_cc_sweep(const int* faces, int64_t n_faces, int64_t n_verts, int* labels, int* changed, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh clean-up: simplification by vertex clustering with quadric-error placement  (csrc/meshclean.hip)
 * (Lindstrom 2000, DeCoro-Tatarchuk 2007.)  One output vertex per occupied cell of a grid of cubes of side `cell` (float32,
 * positive, finite) at `origin` (3 finite float32, HOST pointers below).  No atomics and no contraction anywhere: a cluster's
 * sums belong to one thread, which adds in the order stated, so two runs agree bit for bit and a float64 restatement in the
 * same order (tests/mesh_clean_ref.py) can differ in the last float32 rounding only.
 *
 * 1. Keys (mnr_mesh_cluster_keys), per vertex v and axis a, float32 in this order: q_a = floor((x_a - origin_a) / cell),
 *    c_a = int(q_a).  keys[v] = (c_0 << 42) | (c_1 << 21) | c_2 as int64; MNR_MESH_KEY_NONFINITE where a coordinate is not
 *    finite, else MNR_MESH_KEY_OUTSIDE where some q_a is outside [0, MNR_MESH_CELL_LIMIT).  The caller refuses a mesh with a
 *    negative key.
 * 2. The caller: the distinct keys in ascending order are the clusters, output vertex k is the k-th of them, map[v] is the rank
 *    of keys[v]; members = the vertex ids stably sorted by map (a cluster's members in ascending id), member_start
 *    [n_clusters + 1] their offsets.
 * 3. Faces (mnr_mesh_cluster_faces), per face f = (a, b, c): mapped[f] = (map[a], map[b], map[c]); canon[f] = mapped[f] rotated
 *    so that its smallest entry comes first (the first of equal ones); keep[f] = 1 iff the three clusters are distinct;
 *    incident[f] = (map[a]; map[b] or -1 if it equals map[a]; map[c] or -1 if it equals map[a] or map[b]): each cluster the
 *    face touches, once.  A face with an index outside [0, n_verts), or a map entry outside [0, n_clusters), gets -1
 *    everywhere and keep 0.
 * 4. The caller: cluster_faces = the face ids of the incident entries != -1, stably sorted by cluster from face-major order (a
 *    cluster's faces in ascending id, each once), face_start [n_clusters + 1] their offsets, n_incident their number.  The
 *    output faces are mapped[f] for the f with keep[f] = 1 that are the lowest id among the faces with the same canon[f], in
 *    ascending f: order and winding survive, and of two faces that are the same directed triple up to rotation the first
 *    stays.  Two coincident faces of OPPOSITE winding both stay.
 * 5. Clusters (mnr_mesh_cluster_solve), one thread per cluster k, float64 throughout, inputs widened from float32:
 *    m_a = origin_a + cell (c_a + 0.5) is the cell's centre (c_a from keys[k]); every coordinate below is relative to it,
 *    p = double(vertex) - m.
 *    members v in list order:  sg += p_v,  sn += normal_v,  sc += colour_v (integers),  count += 1.
 *    g = sg / count.
 *    faces f = (a, b, c) in list order:  e1 = p_b - p_a, e2 = p_c - p_a,
 *      n = (e1_1 e2_2 - e1_2 e2_1, e1_2 e2_0 - e1_0 e2_2, e1_0 e2_1 - e1_1 e2_0),  L = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2);
 *      the face is skipped unless 0 < L < inf;  d = (n_0 p_a0 + n_1 p_a1) + n_2 p_a2;
 *      A_ij += (n_i n_j) / L for ij = 00, 01, 02, 11, 12, 22;  r_i += (n_i d) / L.
 *      (E(x) = sum L (n/L . (x - p_a))^2, area-weighted, is x^T A x - 2 r^T x + const.)
 *    tr = (A_00 + A_11) + A_22;  lam = (MNR_QEM_REG tr) / 3;  M = A + lam I;  b_i = r_i + lam g_i.
 *    Closed-form solve by COFACTORS (adjugate over determinant):
 *      c00 = M11 M22 - M12 M12, c01 = M02 M12 - M01 M22, c02 = M01 M12 - M02 M11,
 *      c11 = M00 M22 - M02 M02, c12 = M01 M02 - M00 M12, c22 = M00 M11 - M01 M01,
 *      det = (M00 c00 + M01 c01) + M02 c02,
 *      x_0 = ((c00 b_0 + c01 b_1) + c02 b_2) / det, x_1 = ((c01 b_0 + c11 b_1) + c12 b_2) / det,
 *      x_2 = ((c02 b_0 + c12 b_1) + c22 b_2) / det.
 *    x is taken iff tr > 0, x is finite and |x_a| <= cell / 2 on every axis; otherwise x = g (fallback[k] = 1).
 *    out_verts[k] = float32(m + x).  out_normals[k] = float32(sn / len), len = sqrt((sn_0 sn_0 + sn_1 sn_1) + sn_2 sn_2), or 0
 *    unless 0 < len < inf.  out_colors[k] = (2 sc + count) / (2 count) in integers (the mean, halves rounded up).
 *    MNR_QEM_REG is a decision, not a derived number: lam bounds the condition number of M by about 3 / MNR_QEM_REG, and where
 *    the surface is flat (A of rank 1 or 2) it pulls the solution toward the centroid instead of letting it slide along
 *    the plane.  The minimiser of E + lam |x - g|^2 cannot have a larger E than g, and the fallback is g: E(x) <= E(g).
 *    Entries of members / cluster_faces / faces outside their ranges are skipped and the offsets are clipped to their lists: no
 *    access leaves the inputs or row k of the outputs.
 * n_verts == 0, n_faces == 0, n_clusters == 0 are successful no-ops of the entries they size.
 * ------------------------------------------------------------------------- */
#define MNR_QEM_REG 1e-3
#define MNR_MESH_CELL_LIMIT (1 << 21)
#define MNR_MESH_KEY_NONFINITE (-1)
#define MNR_MESH_KEY_OUTSIDE (-2)
typedef struct {
  int64_t n_clusters, n_verts, n_faces, n_incident;
  const float* verts;              /* [n_verts,3] */
  const float* normals;            /* [n_verts,3] */
  const unsigned char* colors;     /* [n_verts,3] or NULL */
  const int* faces;                /* [n_faces,3] */
  const int64_t* keys;             /* [n_clusters]: the distinct keys, ascending */
  const int64_t* member_start;     /* [n_clusters + 1] */
  const int* members;              /* [n_verts] */
  const int64_t* face_start;       /* [n_clusters + 1] */
  const int* cluster_faces;        /* [n_incident] */
  float origin[3];
  float cell;
  float* out_verts;                /* [n_clusters,3] */
  float* out_normals;              /* [n_clusters,3] */
  unsigned char* out_colors;       /* [n_clusters,3] or NULL (colors and out_colors: both or neither) */
  unsigned char* fallback;         /* [n_clusters] or NULL */
} mnr_mesh_cluster_args;
int mnr_mesh_cluster_keys(const float* verts, int64_t n_verts, const float* origin, float cell, int64_t* keys, void* stream);
int mnr_mesh_cluster_faces(const int* faces, int64_t n_faces, const int* map, int64_t n_verts, int64_t n_clusters, int* mapped,
                           int* canon, int* incident, unsigned char* keep, void* stream);
int mnr_mesh_cluster_solve(const mnr_mesh_cluster_args* args, void* stream);

/* ------------------------------------------------------------------------- *
 * Texture atlas: per-face charts in a regular grid of cells  (csrc/atlas.hip)
 * A closed-form layout: no chart growing, no packing, no hashing, no atomics, no contraction.  Two runs write the same atlas and
 * a NumPy restatement (tests/atlas_ref.py) follows it exactly.  T = n_faces, c >= MNR_ATLAS_MIN_CELL the cell size in texels.
 *
 * Layout.  Faces 2k and 2k + 1 share cell k; ncells = ceil(T / 2).  A cell is (c + 1) texels wide and c high; cells fill the atlas
 * row-major, `cols` per row: W = cols (c + 1), rows = ceil(ncells / cols), H = rows c (T = 0: W = H = 0).  Row 0 is the TOP row of
 * the image.  The top-left texel of cell k is (X0, Y0) = ((k % cols) (c + 1), (k / cols) c).
 *
 * Ownership.  The local texel (X, Y), X in 0 .. c, Y in 0 .. c - 1, belongs to the lower face 2k iff X + Y <= c - 1 and to the upper
 * face 2k + 1 otherwise: c (c + 1) / 2 texels each, every texel of a cell has exactly one owner.  The upper half is the lower half
 * rotated by 180 degrees about the cell's centre.  In FACE-LOCAL texels (x', y'), x', y' >= 0, x' + y' <= c - 1:
 *   lower  (x', y') = (X, Y)                    i.e. texel (X0 + x', Y0 + y')
 *   upper  (x', y') = (c - X, c - 1 - Y)        i.e. texel (X0 + c - x', Y0 + c - 1 - y')
 * so a face's chart is one anchor texel (its v0) and a step of +1 (lower) or -1 (upper) along both axes.
 *
 * Texel to surface (mnr_atlas_samples), float32 in the order written:
 *   b1 = float(x') / float(c - 2),  b2 = float(y') / float(c - 2),  b0 = (1 - b1) - b2,  p = (b0 v0 + b1 v1) + b2 v2.
 * v0 is the texel x' = y' = 0, v1 the texel x' = c - 2, v2 the texel y' = c - 2.  The texels with x' + y' = c - 1 (and so those with
 * x' = c - 1 or y' = c - 1) lie just outside the triangle, b0 < 0: they are the GUTTER, baked at the extrapolated point of the
 * face's plane and not dilated afterwards.
 *
 * Surface to UV (mnr_atlas_uvs).  Texel centres are at + 0.5; the pixel position of the barycentric point (b0, b1, b2) is the centre
 * of the anchor texel plus or minus (c - 2) (b1, b2).  With x' = c - 2 for v1 and y' = c - 2 for v2 in the two rows above:
 *          v0                         v1                           v2
 *   lower  (X0 + .5,     Y0 + .5)     (X0 + c - 1.5, Y0 + .5)      (X0 + .5,     Y0 + c - 1.5)      = X0 + x' + .5, Y0 + y' + .5
 *   upper  (X0 + c + .5, Y0 + c - .5) (X0 + 2.5,     Y0 + c - .5)  (X0 + c + .5, Y0 + 1.5)          = X0 + c - x' + .5, Y0 + c - 1 - y' + .5
 *   u = px / float(W),  v = 1 - py / float(H)   (float32; v = 1 is the top of the image).
 * The UV triangle is the owned region shrunk by one texel from the hypotenuse, which makes the texture seam-safe WITHOUT padding:
 * a bilinear lookup at s = (c - 2) b1, t = (c - 2) b2 (s, t >= 0, s + t <= c - 2) reads the face-local texels (i, j), (i + 1, j),
 * (i, j + 1), (i + 1, j + 1) with i = floor(s), j = floor(t).  i + j <= c - 2, so the first three have x' + y' <= c - 1: owned.  The
 * fourth is not owned only if i + j = c - 2, which needs s + t = c - 2 with s = i and t = j: both fractions are 0 and its weight
 * is exactly 0.  (In exact arithmetic: a UV rounded to float32 is off by up to 2^-24 of itself, a weight of that order.)
 *
 * Footprint.  A texel is the parallelogram spanned by a = (v1 - v0) / float(c - 2) and b = (v2 - v0) / float(c - 2) (float32).  The
 * Gaussian with the moments of the uniform distribution over it, scaled by the filter width, has mean p and
 *   cov_ij = cov_scale (a_i a_j + b_i b_j),  cov_scale = filter^2 / 12 (float64 on the host, passed as a float; 0: point samples).
 * The covariance has rank 2: flat along the normal.  mnr_ipe_from_gaussians takes it as it is.
 *
 * Normal and view direction.  n = (b0 n0 + b1 n1) + b2 n2 over len = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2) where 0 < len < inf; else
 * the face normal g = (v1 - v0) x (v2 - v0), g_0 = e1_1 e2_2 - e1_2 e2_1 and cyclic, over its length under the same condition;
 * else (0, 0, 1).  viewdir = -n; with the last fallback the view direction is (0, 0, 1) too.
 *
 * Invalid samples: the upper half of the last cell when T is odd; a face with a vertex position that is not finite (or an index
 * outside [0, n_verts)); a sample whose mean or covariance is not finite in float32.  They get zero mean and covariance, normal
 * and view direction (0, 0, 1) and face = -1; mnr_atlas_store skips them, so their texels keep what the caller put there and the
 * mask stays as it was.  Every output is finite.
 *
 * Samples are numbered s = cell c (c + 1) + Y (c + 1) + X, the total is ncells c (c + 1) (int64).  A chunk [s0, s0 + n) is any range
 * of them, n < 2^31: memory is bounded by the chunk, not by the atlas.
 *   mnr_atlas_samples  one thread per sample: means [n,3], covs [n,3,3], normals [n,3], viewdirs [n,3], face [n] (76 B a sample).
 *   mnr_atlas_store    per sample with face >= 0: atlas[Y0 + Y, X0 + X] = floor(clip(rgb, 0, 1) * 255 + 0.5) (NaN counts as 0),
 *                      mask = 255 there, and atlas_f32 (when given) the rgb as it came.  One sample per texel: no atomics.
 *   mnr_atlas_uvs      uv [T,3,2]: (u, v) of v0, v1, v2 of every face.  Reads only c, cols, W, H and n_faces.
 * ------------------------------------------------------------------------- */
#define MNR_ATLAS_MIN_CELL 3
typedef struct {
  const float* verts;              /* [n_verts,3] */
  const float* normals;            /* [n_verts,3] */
  const int* faces;                /* [n_faces,3] */
  int64_t n_verts, n_faces;
  int c;                           /* cell size in texels, >= MNR_ATLAS_MIN_CELL */
  int cols;                        /* cells per atlas row, >= 1 */
  int W, H;                        /* cols (c + 1) and ceil(ceil(n_faces / 2) / cols) c; both 0 when n_faces == 0 */
  float cov_scale;                 /* filter^2 / 12, finite and >= 0 */
} mnr_atlas_args;
int mnr_atlas_samples(const mnr_atlas_args* args, int64_t s0, int64_t n, float* means, float* covs, float* normals, float* viewdirs,
                      int* face, void* stream);
int mnr_atlas_store(const mnr_atlas_args* args, int64_t s0, int64_t n, const float* rgb, const int* face, unsigned char* atlas,
                    unsigned char* mask, float* atlas_f32, void* stream);
int mnr_atlas_uvs(const mnr_atlas_args* args, float* uv, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh rasteriser: a visibility buffer and its shading  (csrc/raster.hip)
 * 2D homogeneous rasterisation (Olano and Greer 1997): the edge functions come from the homogeneous vertices, nothing is clipped,
 * and a triangle that crosses the camera plane is no special case.  proj [3,4] is the matrix of the TSDF section (mesh.world_to_pixel):
 * P (X, 1) = (u zc, v zc, zc), pixel (x, y) has its centre at (x + .5, y + .5) and zc is the rendered distance.  Everything is float32
 * in the order written, no contraction; a NumPy restatement (tests/raster_ref.py) follows it exactly, every face against every pixel.
 *
 * Per vertex  h_v[r] = ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3], r = 0, 1, 2: it depends on the vertex only, so every face
 *             that uses a vertex sees the same three numbers.
 * Per face    (corners 0, 1, 2; (i, j, k) cyclic)  n_i = h_j x h_k, i.e. n_i.x = h_j.y h_k.z - h_j.z h_k.y, n_i.y = h_j.z h_k.x -
 *             h_j.x h_k.z, n_i.z = h_j.x h_k.y - h_j.y h_k.x;  det = (n_0.x h_0.x + n_0.y h_0.y) + n_0.z h_0.z;  s = sign(det).
 *             A face is SKIPPED if it has an index outside [0, n_verts), a coordinate of h that is not finite, or a det that is 0
 *             or not finite; with cull = MNR_RASTER_CULL_BACK also if det > 0 (see `front` below).
 * Per pixel   E_i = ((s n_i.x)(x + .5) + (s n_i.y)(y + .5)) + s n_i.z;  S = (E_0 + E_1) + E_2;  zc = |det| / S.
 * Covered     iff for every i: E_i > 0, or E_i == 0 and tie(s n_i);  and S > 0;  and zc is finite;  and zc > near;  and the pixel
 *             lies in the face's pixel box (below).  tie(a, b, c) = a > 0 or (a == 0 and (b > 0 or (b == 0 and c > 0))).
 * Resolve     vis[y, x] = the minimum of key = (bits(zc) << 32) | face over the covering faces (zc > 0: its bit pattern is
 *             monotone; the nearest face wins, among equal depths the lowest id); all ones where no face covers the pixel.
 *
 * Why this form.  The face across an edge computes h_k x h_j, which without contraction is exactly -n_i, so for two faces of one
 * orientation a pixel centre is on opposite sides of the shared edge, or exactly on it for both, and then tie() gives it to exactly
 * one: no cracks and no double hits across an edge, by construction.  E_i / S are the perspective-correct barycentrics, |det| / S
 * is the zc of the surface point, and S > 0 with every E_i >= 0 implies that the point lies in front of the camera plane.
 * LIMIT.  The argument is per EDGE.  Where a vertex of a fan projects within rounding of a pixel centre, the fan's rounded edge
 * lines need not meet in one point and that one pixel can be claimed by no face of the fan, or by several.  Curing it needs vertices
 * snapped to fixed point, which cannot represent a vertex behind the camera; it is not done.
 * `front`.  For a P whose left 3 x 3 block has a positive determinant (world_to_pixel's always has: K diag(1, -1, -1) R^T with
 * det K > 0) a face whose corners run counter-clockwise seen from the camera, i.e. whose geometric normal (v1 - v0) x (v2 - v0)
 * faces the camera, has det < 0: the flip of y makes pixel space left-handed as seen on the screen.  MNR_RASTER_CULL_BACK keeps
 * exactly those.
 *
 * Pixel box.  If all three h.z > 0: with a = h.x / h.z (h.y / h.z) of the three corners (float32 divisions), the columns (rows)
 * max(floor(min a) - 1, 0) .. min(floor(max a) + 1, W - 1 (H - 1)), none if that is empty.  If all three h.z <= 0 (the face lies
 * wholly behind the camera plane): none.  Otherwise (it crosses the plane): the whole image.  In exact arithmetic a covered centre
 * lies inside the box of the projected corners, the pixel of margin keeps the rounding of a and of well-conditioned edge
 * functions from excluding one, and a face behind the plane covers nothing: sum_i E_i h_i.z = |det| > 0 needs an h_i.z > 0.  The box is nevertheless a CLAUSE of the coverage test and not only a
 * prune: the edge functions of a sliver are differences of products that cancel almost completely, their signs far from the
 * sliver are rounding noise, and without the clause such a face claims stray pixels with a meaningless zc (a face of 0.001 pixel
 * of a 10364-face sphere claimed a pixel 1.8 pixels away, in front of everything).  Inside its box a sliver's coverage and zc
 * remain noise; and where the noise of an edge exceeds the pixel of margin (|u|, |v| far beyond 10^4) the clause can open a crack.
 * A face whose box holds more than `threshold` pixels takes the large-face path (a workgroup per face), the others
 * the small-face path (a thread per face); both run the same coverage function, so threshold = 0 (all large), any value in
 * between and a huge one (all small) write the same buffer bit for bit.  list [n_faces] and count [1] are the workspace of the
 * large-face list; what they hold afterwards is not specified (the list's order depends on arrival, the buffer does not).
 * The only atomics are integer: a 64-bit unsigned atomicMin per covered pixel and an atomicAdd per wave for the list.
 *
 * mnr_raster_visibility fills vis [H,W] and resolves.  mnr_raster_shade, a thread a pixel, decodes the winner f, recomputes E_i, S
 * and zc (the same code, the same bits) and writes, with l_i = E_i / S:
 *   face [H,W] = f, depth [H,W] = zc, acc [H,W] = 1, bary [H,W,3] = l;
 *   normals [H,W,3]: n = (l_0 n_0 + l_1 n_1) + l_2 n_2 of the vertex normals over len = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2) where
 *     0 < len < inf; else the face normal (v1 - v0) x (v2 - v0) (the atlas section's formula) over its length under the same
 *     condition; else (0, 0, 1);
 *   rgb [H,W,3]: with colors [n_verts,3] (uint8: c / 255.f first) c = (l_0 c_0 + l_1 c_1) + l_2 c_2.
 *     With texture [Ht,Wt,3] (uint8: t / 255.f first) and uv [n_faces,3,2] (u, v of each face's corners, v = 1 the top row, what
 *     mnr_atlas_uvs writes): (u, v) blended like c;  x = u float(Wt) - .5, y = (1 - v) float(Ht) - .5;  xf = floor(x), fx = x - xf,
 *     columns xa = clamp(int(xf), 0, Wt - 1) and xb = clamp(int(xf) + 1, 0, Wt - 1), rows ya, yb likewise;
 *     top = (1 - fx) t[ya,xa] + fx t[ya,xb],  bot = (1 - fx) t[yb,xa] + fx t[yb,xb],  rgb = (1 - fy) top + fy bot.
 *     With neither: the shaded normal 0.5 + 0.5 n.  colors and texture together are refused.
 * A pixel without a winner (all ones, or a key that names no rasterisable face) gets face -1, depth 0, acc 0, bary 0, normals 0 and
 * rgb = bg.  depth and acc are what mnr_tsdf_integrate takes.  n_faces == 0: the buffer is filled and nothing else is launched.
 * H, W >= 1; near > 0 and finite; n_faces < 2^31 - 1.
 * ------------------------------------------------------------------------- */
#define MNR_RASTER_CULL_NONE 0
#define MNR_RASTER_CULL_BACK 1
typedef struct {
  const float* verts;              /* [n_verts,3] */
  const float* normals;            /* [n_verts,3] (shade) */
  const int* faces;                /* [n_faces,3] */
  int64_t n_verts, n_faces;
  float proj[12];                  /* [3,4], row-major */
  int H, W;
  float near;                      /* > 0, finite */
  int cull;                        /* MNR_RASTER_CULL_* (visibility) */
  int64_t threshold;               /* >= 0: box pixels above which a face takes the large-face path (visibility) */
  const void* colors;              /* [n_verts,3] float or uint8, or NULL (shade) */
  int colors_u8;
  const void* texture;             /* [Ht,Wt,3] float or uint8, or NULL (shade) */
  int texture_u8;
  int Ht, Wt;
  const float* uv;                 /* [n_faces,3,2], with a texture (shade) */
  float bg[3];
} mnr_raster_args;
int mnr_raster_visibility(const mnr_raster_args* args, uint64_t* vis, int* list, int* count, void* stream);
int mnr_raster_shade(const mnr_raster_args* args, const uint64_t* vis, int* face, float* depth, float* acc, float* bary, float* normals,
                     float* rgb, void* stream);

/* ------------------------------------------------------------------------- *
 * View-dependent texture: a per-texel spherical-harmonic fit and its shading  (csrc/shtex.hip)
 * A texel holds K = (L + 1)^2 real SH coefficients per channel, L in 0 .. MNR_SHTEX_MAX_DEGREE, fitted to the colours of D fixed
 * WORLD directions by weighted ridge least squares over the hemisphere the texel can be seen from, and the shading pass evaluates
 * them at each pixel's own view direction.  Everything is float32 in the order written unless it says float64, no contraction;
 * tests/shtex_ref.py restates it in NumPy.  dot, sub and normalise are csrc/mesh_math.h's (the sections above spell them out).  A view
 * direction points from the eye TO the surface: a direction d sees a surface of unit normal n iff dot(d, n) < 0.
 *
 * Basis (index, then the usual name), of a unit direction (x, y, z), without the Condon-Shortley phase:
 *   0  C0                1  C1 y              2  C1 z              3  C1 x
 *   4  C2A (x y)         5  C2A (y z)         6  C2B (3 (z z) - 1) 7  C2A (x z)         8  C2C (x x - y y)
 * with the products in parentheses first.  The constants are the literals below (sqrt(1 / 4 pi), sqrt(3 / 4 pi), sqrt(15 / 4 pi),
 * sqrt(5 / 16 pi), sqrt(15 / 16 pi)).  There are two evaluations of these formulas: the host table Y [D,K] in float64 (Python, from
 * the float32 directions converted to float64, the constants as float64), which the fit reads; and a float32 __device__ function
 * (the constants rounded to float32) in the shading pass.
 *
 * Weight.  a = -dot(d_k, n);  w_k = a > 0 ? (a < 1 ? a : 1) : 0, i.e. min(max(a, 0), 1) with NaN and -0 mapped to +0.
 *   mnr_shtex_weights  one thread per pair: w [n,D] of dirs [D,3] and normals [n,3].
 *
 * Fit (mnr_shtex_fit), one thread per texel, float64 from here on; w_k, rgb_kc and lam are converted to float64 exactly.
 *   A direction is USED iff w_k > 0 and the three values rgb_k. are finite; the rgb of a direction with w_k == 0 is not read.
 *   Over the used k ascending, for i = 0 .. K - 1:  t = w_k Y_ki;  M_ij += t Y_kj for j = i .. K - 1;  b_ic += t rgb_kc for c = 0, 1, 2;
 *   and sw += w_k, s_c += w_k rgb_kc.  (All sums start at +0.)
 *   tr = ((M_00 + M_11) + ...) + M_{K-1,K-1};  mu = (lam tr) / K;  M_ii += mu for i >= 1: the constant term is not regularised.
 *   Cholesky M = G G^T, rows i = 0 .. K - 1, in a row j = 0 .. i:  s = M_ji;  s -= G_ip G_jp for p = 0 .. j - 1 ascending;
 *     j < i: G_ij = s / G_jj;   j == i: the PIVOT s must be > 0 and finite, G_ii = sqrt(s).
 *   Per channel:  forward  s = b_ic;  s -= G_ip y_p for p = 0 .. i - 1 ascending;  y_i = s / G_ii   (i ascending);
 *                 back     s = y_i;   s -= G_pi x_p for p = i + 1 .. K - 1 ascending;  x_i = s / G_ii   (i descending).
 *   coef_ic = float32(x_ic), rounded once.
 *   Fallbacks.  No direction used: every coefficient is 0.  A pivot that is <= 0 or not finite, or a coef that is not finite in
 *   float32: coef_0c = float32((s_c / sw) / Y_00) (Y_00 the table's first entry; 0 if that is not finite in float32), the other
 *   coefficients 0: the weighted mean colour as a constant.  Every output is finite.
 *   No atomics and no reduction across threads: two runs give the same bits.  The 45 + 27 + 4 sums of degree 2 live in float64
 *   registers; Y is staged in LDS (D K doubles, every lane reads the same address: a broadcast), so D <= MNR_SHTEX_MAX_DIRS.
 *
 * Shade (mnr_shtex_shade), one thread per pixel, reads face [H,W] and bary [H,W,3] as mnr_raster_shade wrote them.  For a pixel
 * with 0 <= face < n_faces whose three indices lie inside the vertices (any other pixel is left untouched and keeps `bg`):
 *   X = (l_0 v_0 + l_1 v_1) + l_2 v_2;   d = normalise(X - origin), (0, 0, 1) where the length is 0 or not finite;
 *   (u, v), x, y, fx, fy, xa, xb, ya, yb exactly as in the rasteriser's texture lookup above, on sh [Ht,Wt,K,3] float32;
 *   per coefficient j and channel c the plane is interpolated in that form:  top = (1 - fx) t[ya,xa] + fx t[ya,xb],  bot likewise
 *   on row yb,  v_jc = (1 - fy) top + fy bot;
 *   r_c = Y_0(d) v_0c, then r_c = r_c + Y_j(d) v_jc for j = 1 .. K - 1 ascending;   rgb_c = r_c > 0 ? (r_c < 1 ? r_c : 1) : 0 (NaN: 0).
 * ------------------------------------------------------------------------- */
#define MNR_SHTEX_MAX_DEGREE 2
#define MNR_SHTEX_MAX_DIRS 512
#define MNR_SH_C0 0.28209479177387814
#define MNR_SH_C1 0.4886025119029199
#define MNR_SH_C2A 1.0925484305920792
#define MNR_SH_C2B 0.31539156525252005
#define MNR_SH_C2C 0.5462742152960396
int mnr_shtex_weights(const float* dirs, int64_t n_dirs, const float* normals, int64_t n, float* w, void* stream);
int mnr_shtex_fit(const float* dirs, const double* Y, int64_t n_dirs, int degree, const float* normals, const float* rgb, int64_t n,
                  double lam, float* coef, void* stream);
typedef struct {
  const float* verts;              /* [n_verts,3] */
  const int* faces;                /* [n_faces,3] */
  int64_t n_verts, n_faces;
  const int* face;                 /* [H,W], mnr_raster_shade's */
  const float* bary;               /* [H,W,3], mnr_raster_shade's */
  int H, W;
  const float* uv;                 /* [n_faces,3,2] */
  const float* sh;                 /* [Ht,Wt,K,3], K = (degree + 1)^2 */
  int Ht, Wt;                      /* 1 .. 2^24 each */
  int degree;                      /* 0 .. MNR_SHTEX_MAX_DEGREE */
  float origin[3];                 /* the eye, finite */
} mnr_shtex_shade_args;
int mnr_shtex_shade(const mnr_shtex_shade_args* args, float* rgb, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh geometry: point-to-mesh distance over a uniform grid, surface sampling  (csrc/meshdist.hip)
 * Everything is float32 in the order written unless it says float64, no contraction; tests/geometry_ref.py restates it in NumPy,
 * every query against every face.  dot(x, y) = (x_0 y_0 + x_1 y_1) + x_2 y_2;  cross(u, v) = (u_1 v_2 - u_2 v_1, u_2 v_0 - u_0 v_2,
 * u_0 v_1 - u_1 v_0);  min is fminf.  A face is VALID iff its three indices lie in [0, n_verts) and its nine coordinates are
 * finite; every kernel below skips a face that is not.  A point cloud is a mesh whose faces are (i, i, i).
 *
 * Squared distance of a point p to a face (a, b, c):
 *   seg(p, u, v):  uv = v - u, up = p - u, L = dot(uv, uv);  t = min(max(dot(up, uv) / L, 0), 1) if L > 0, else 0;
 *                  e = up - t uv (the products first, then the subtractions);  dot(e, e).
 *   d2 = min(min(seg(p, a, b), seg(p, b, c)), seg(p, c, a)).
 *   ab = b - a, ac = c - a, n = cross(ab, ac), nn = dot(n, n).  If nn > 0, with ap = p - a, bp = p - b, cp = p - c, bc = c - b, ca = a - c:
 *   s_0 = dot(n, cross(ab, ap)), s_1 = dot(n, cross(bc, bp)), s_2 = dot(n, cross(ca, cp));  if s_0 >= 0 and s_1 >= 0 and s_2 >= 0:
 *   h = dot(n, ap), d2 = min(d2, (h h) / nn).
 * Why this form and not the closest-point routine that walks the seven Voronoi regions with unguarded quotients: that one returns
 * NaN for a face with two equal corners, is wrong by the size of the scene for three collinear corners, and differs from its own
 * float64 evaluation by 2e-2 on slivers.  Here three equal corners are a point and collinear corners a segment without a special
 * case, and the plane term, a lower bound of the true distance wherever it is taken, can only be taken over the prism of the face.
 * LIMIT.  The normal of a sliver whose height is within rounding of its corners (about 1e-7 of their size) is rounding noise; for
 * a query that lies within rounding of the plane through the sliver's long edge and that noise, the three signs can pass and
 * (h h) / nn can then be far below the true distance.
 *
 * Result per query: the minimum of key = (bits(d2) << 32) | face over the ELIGIBLE faces, d2 >= 0 so its bit pattern is monotone
 * (the rasteriser's resolve): d2 [n] float32 the smallest squared distance, face [n] int32 the lowest face id that attains it.  A
 * face is eligible iff it is valid and d2 <= lim, lim = max_dist max_dist in float32 (max_dist > 0; +inf: every valid face; a d2
 * that is NaN is not eligible).  No eligible face, or a query with a coordinate that is not finite: d2 = +inf, face = -1.  The
 * result does not depend on the order of traversal, hence not on the grid: two runs, and two grids, agree bit for bit.
 *
 * Grid.  Cubes of side `cell` (> 0, finite) at `origin`, dims [3] cells, dims_a in [1, MNR_MESHDIST_MAX_DIM]; cell (x, y, z) has
 * the linear index (x dims_1 + y) dims_2 + z.  A coordinate v of axis a lies in cell(v) = int(min(max(floor((v - origin_a) / cell),
 * 0), dims_a - 1)) (the clamps as float; that function does not decrease in v).  The caller sets origin and `hi` to the
 * per-axis minimum and maximum over the corners of the valid faces (exactly) and dims_a = cell(hi_a) + 1.
 *   mnr_mesh_grid_count  counts[f] (int64) = the number of cells the box of face f overlaps, prod_a (cell(max_a) - cell(min_a) + 1)
 *                        with min_a / max_a over its three corners; 0 for a face that is not valid.
 *   mnr_mesh_grid_fill   with offsets [n_faces + 1] (int64) the exclusive scan of counts and n_pairs its last entry: face f writes
 *                        (cell, f) into pair_cell / pair_face [n_pairs] (int32) from offsets[f] on, x outermost, z innermost; no
 *                        atomics, nothing outside [offsets[f], min(offsets[f + 1], n_pairs)).
 *   The caller sorts the pairs stably by cell (a cell's faces ascending) and builds cell_start [cells + 1] (int64).
 *   mnr_mesh_distance    one thread a query; with `order` [n] (int64, or NULL) thread t serves query order[t], so that the caller
 *                        can sort the queries by cell and still gets the results in its own order.  With q = min(max(p, origin), hi)
 *                        per axis, g_a = (q_a - origin_a) / cell, c_a = cell(q_a), fr_a = min(max(g_a - c_a, 0), 1) and
 *                        out2 = dot(ex, ex), ex_a = max(max(origin_a - p_a, p_a - hi_a), 0), the thread visits the Chebyshev shells
 *                        r = 0, 1, 2, ... of cells around c (clipped to the grid), every face of every cell, and stops after shell r
 *                        when no side of the cube of shells <= r lies inside the grid any more, or else, with m the smallest of
 *                        fr_a over the axes with c_a - r > 0 and 1 - fr_a over those with c_a + r < dims_a - 1,
 *                          bound = cell max((float(r) + m) - MNR_MESHDIST_MARGIN, 0),  lb2 = (out2 + bound bound) MNR_MESHDIST_SHRINK,
 *                        when best d2 < lb2 or lb2 > lim.  csrc/meshdist.hip argues why every face not yet seen then has a
 *                        COMPUTED d2 of at least lb2.  shells [n] (int32, or NULL) receives the number of shells visited.
 *   cell_start entries outside [0, n_pairs], pair_face entries outside [0, n_faces), face indices outside the vertices and entries
 *   of order outside [0, n) are skipped: no access leaves the inputs.  n == 0, or n_pairs == 0: nothing to visit, every query gets
 *   the empty result.
 *
 * Sampling.  mnr_mesh_face_areas: area[f] (float64) = 0.5 sqrt(dot(n, n)), n = cross(b - a, c - a) with the float32 corners widened
 * first; 0 for a face that is not valid.  mnr_mesh_sample, one thread a sample i of n (n < 2^31), given cum [n_faces] (float64), the
 * caller's inclusive running sum of the areas (an input: the order of that sum is not part of the contract):
 *   u = ((double(i) + 0.5) / double(n)) cum[n_faces - 1];  k = the first face with cum[k] > u (binary search; n_faces - 1 if none).
 *   mix(x), uint32 arithmetic:  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16.
 *   s = mix(seed), h_1 = mix(s + 2 i), h_2 = mix(s + (2 i + 1));  r_j = float(h_j >> 8) 2^-24 (exact).
 *   If r_1 > 1 - r_2 (that is r_1 + r_2 > 1, evaluated without a rounding): r_1 = 1 - r_1, r_2 = 1 - r_2.
 *   b = ((1 - r_1) - r_2, r_1, r_2) (exact, every entry in [0, 1]);  point = (b_0 a + b_1 b) + b_2 c;  face[i] = k.
 * Stratified in the area, no square root, no rejection.  A k that names no valid face gives face -1 and the point 0.
 * ------------------------------------------------------------------------- */
#define MNR_MESHDIST_MAX_DIM 1024
#define MNR_MESHDIST_MARGIN 0.03125f            /* 2^-5 of a cell */
#define MNR_MESHDIST_SHRINK 0.9999847412109375f /* 1 - 2^-16 */
#define MNR_MESHRAY_MARGIN 0.03125f              /* 2^-5 of a cell: the ray caster's walk ("Mesh ray casting" below) */
#define MNR_MESHRAY_REL 3.814697265625e-06f      /* 2^-18 = 64 float32 ulps, of R (there) */
typedef struct {
  const float* verts;              /* [n_verts,3] */
  const int* faces;                /* [n_faces,3] */
  int64_t n_verts, n_faces;
  float origin[3];
  float hi[3];
  float cell;
  int dims[3];
} mnr_meshdist_args;
int mnr_mesh_grid_count(const mnr_meshdist_args* args, int64_t* counts, void* stream);
int mnr_mesh_grid_fill(const mnr_meshdist_args* args, const int64_t* offsets, int64_t n_pairs, int* pair_cell, int* pair_face,
                       void* stream);
int mnr_mesh_distance(const mnr_meshdist_args* args, const int64_t* cell_start, const int* pair_face, int64_t n_pairs,
                      const float* points, const int64_t* order, int64_t n, float max_dist, float* d2, int* face, int* shells,
                      void* stream);
int mnr_mesh_face_areas(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, double* area, void* stream);
int mnr_mesh_sample(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, const double* cum, int64_t n,
                    uint32_t seed, float* points, int* face, void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh registration: closest points, ICP normal equations, polygonal crop volumes  (csrc/meshreg.hip)
 * The notation, the validity of a face and the distance formula are those of "Mesh geometry" above; float32 in the order written
 * unless it says float64, no contraction; tests/registration_ref.py restates everything in NumPy.  No atomics and no reduction
 * whose order depends on scheduling: two runs agree bit for bit.
 *
 * mnr_mesh_closest, one thread a query i of n (n < 2^31): given points [n,3] and face [n] (int32, what mnr_mesh_distance returned;
 * -1: none) it writes x [n,3], the closest point of the face, and nrm [n,3], the face's unit normal, from the terms of the
 * distance formula:
 *   q = (seg(p, a, b), seg(p, b, c), seg(p, c, a));  k = the lowest index of the smallest q (start at 0, replace on <), m = q_k;
 *   with (u, v) the ends of segment k and t its clamped parameter (seg's own t):  x = u + t (v - u)  (difference, product, sum).
 *   n = cross(b - a, c - a), nn = dot(n, n).  If nn > 0 and s_0 >= 0 and s_1 >= 0 and s_2 >= 0 (the three signs of the distance formula), with h = dot(n, p - a):
 *   if (h h) / nn <= m:  x = p - (h / nn) n  (quotient, products, differences).
 *   nrm = n / sqrt(nn) (sqrt and three quotients) if nn > 0 and finite, else 0.
 * So x is the foot of the term that gave d2 (the plane term on a tie), and |p - x|^2 is that d2 up to the rounding of forming x.
 * With vnormals [n_verts,3] (float32, or NULL) a face (i, i, i), a cloud's point, takes nrm = vnormals[i] / |vnormals[i]| (the length
 * as sqrt(dot), three quotients; 0 if the length is 0 or not finite) in place of the face's.  face[i] outside [0, n_faces), a face
 * that is not valid, or a point with a coordinate that is not finite: x = p, nrm = 0.
 *
 * mnr_mesh_face_normals: nrm [n_faces,3] = n / sqrt(nn) by the same expression; 0 for a face that is not valid, or whose nn is not
 * positive and finite.
 *
 * mnr_icp_sums: over the correspondences i with keep[i] != 0 (uint8 [n], n < 2^31), float64 throughout from the float32 p, x, nrm
 * [n,3] widened first, with `centre` c (double [3] on the HOST, finite), p' = p - c, x' = x - c, d = p - x, r = dot(d, nrm),
 * J = (cross(p', nrm), nrm) (6 entries), out [MNR_ICP_SUMS] (float64) receives the sums of
 *   [0] 1   [1..3] p'   [4..6] x'   [7..15] p'_k x'_l at 7 + 3 k + l   [16] dot(p', p')   [17] dot(x', x')   [18] dot(d, d)   [19] r r
 *   [20..40] J_k J_l for k <= l, row by row ((0,0), (0,1), .. (0,5), (1,1), ..)   [41..46] J_k r.
 * Point to point (Kabsch, Umeyama) needs [0..17], point to plane solves (sum J^T J) xi = -(sum J^T r) for xi = (rotation vector about c,
 * translation); [18] and [19] are the two squared residuals.  The reduction has two levels with nothing left to the scheduler:
 * B = min(ceil(n / 256), 256) workgroups; thread t of workgroup b adds the terms of i = 256 b + t + 256 B k in ascending k; the 256
 * threads' sums of an entry are added as 16 sums of the threads s, 16 + s, .., 240 + s (ascending), s = 0 .. 15, and those 16 in
 * ascending s; `partials`, a workspace of mnr_icp_sums_partials(n) doubles, holds the B results, which are added as four runs of
 * ceil(B / 4) consecutive workgroups (ascending) and those four in order.  n == 0: out = 0.
 *
 * mnr_crop_polygon, one thread a point of n (n < 2^31): keep [n] (uint8) for a polygonal prism, float64 throughout from the float32
 * points widened first.  With (u, v, w) the coordinate indices for the orthogonal `axis` (0 X: 1, 2, 0;  1 Y: 0, 2, 1;  2 Z: 0, 1, 2) and
 * polygon [m,2] (float64, on the device) the corners' (u, v), a point is kept iff w_min <= p_w <= w_max and the number of edges
 * (P_i, P_j), j = i + 1 mod m, with
 *   (P_i.v > p_v) != (P_j.v > p_v)  and  p_u < ((P_j.u - P_i.u) (p_v - P_i.v)) / (P_j.v - P_i.v) + P_i.u
 * is odd.  3 <= m <= MNR_CROP_MAX_POLYGON (every thread walks every edge); a point with a NaN coordinate is not kept.
 * ------------------------------------------------------------------------- */
#define MNR_ICP_SUMS 47
#define MNR_CROP_MAX_POLYGON 4096
int mnr_mesh_closest(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, const float* vnormals, const float* points,
                     const int* face, int64_t n, float* x, float* nrm, void* stream);
int mnr_mesh_face_normals(const float* verts, int64_t n_verts, const int* faces, int64_t n_faces, float* nrm, void* stream);
int mnr_icp_sums_partials(int64_t n);
int mnr_icp_sums(int64_t n, const float* p, const float* x, const float* nrm, const uint8_t* keep, const double* centre, double* partials,
                 double* out, void* stream);
int mnr_crop_polygon(const float* points, int64_t n, const double* polygon, int m, int axis, double w_min, double w_max, uint8_t* keep,
                     void* stream);

/* ------------------------------------------------------------------------- *
 * Mesh ray casting: the nearest ray-triangle intersection over the grid of "Mesh geometry", and its shading  (csrc/meshray.hip)
 * The notation, the validity of a face, cell() and the grid (mnr_mesh_grid_count / mnr_mesh_grid_fill, the caller's sort and cell_start)
 * are those of "Mesh geometry" above.  float32 in the order written unless it says float64, no contraction; tests/raycast_ref.py
 * restates the hit test and the resolve in NumPy, every ray against every face, with no grid.
 *
 * Hit test of a ray (o, d) and a face (a, b, c), the watertight test of Woop, Benthin and Wald (2013); it knows nothing of the grid.
 *   Per ray.   kz = the axis of the largest |d_k| (the lowest index among equal magnitudes);  kx = kz + 1 mod 3, ky = kx + 1 mod 3,
 *              exchanged if d_kz < 0.  Sx = d_kx / d_kz,  Sy = d_ky / d_kz,  Sz = 1 / d_kz.
 *   Per corner.  A = a - o;  Ax = A_kx - Sx A_kz,  Ay = A_ky - Sy A_kz,  Az = Sz A_kz  (the product first);  B and C likewise.
 *   Edge functions, in FLOAT64 from those float32 numbers converted exactly:  U = Cx By - Cy Bx,  V = Ax Cy - Ay Cx,  W = Bx Ay - By Ax.
 *              Each product is exact in float64 and each difference is rounded once, so each sign is exact for the sheared corners.
 *   Inside     iff not ((U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0)): no two have strictly opposite signs, zeros count as
 *              inside;  and det = (U + V) + W is not 0 (a NaN is not 0 here and fails below).  With cull = MNR_RASTER_CULL_BACK also
 *              det > 0: the FRONT faces, whose corners run counter-clockwise seen from the ray origin, i.e. whose geometric normal
 *              (b - a) x (c - a) has a negative product with d: the rasteriser's `front`.
 *   t = float32(((U Az + V Bz) + W Cz) / det)  (float64, Az .. Cz converted exactly, rounded to float32 once).
 *   ELIGIBLE   iff the face is valid, inside, t_min < t <= t_max with t finite (t_max = +inf: no upper limit; a t of +inf or NaN is
 *              never eligible), and the face has AREA: n = cross(b - a, c - a), evaluated in float64 from the corners converted first
 *              (mnr_mesh_face_areas' n), is not (0, 0, 0).  bary = (float32(U / det), float32(V / det), float32(W / det)).
 *   Two faces that share an edge compute the same two sheared corners, so the ray lies on opposite sides of the edge for them, or on it
 *   for both: it is hit by both and never by neither.  Why the area clause: two equal corners give det = 0 for every ray (one edge
 *   function is 0, the other two cancel exactly), but the sheared images of three collinear corners are collinear to rounding only, and
 *   a test that is exact for the sheared corners sees a sliver of that width and lets a ray aimed at it pass.  A face without area in
 *   its own float32 corners is therefore never hit by the clause, not by det; a sliver that has area is a face like any other.
 *   Directions are NOT normalised: t is in units of |d|.
 *
 * Result per ray: the minimum of key = (bits(t) << 32) | face over the eligible faces of the WHOLE mesh (t > t_min >= 0: its bit pattern is
 * monotone; the rasteriser's and the distance query's resolve): t [n] float32, face [n] int32 the lowest id among the nearest hits, bary
 * [n,3] float32 of that face.  No eligible face, a ray with a component of o or d that is not finite, d = 0, or a 1 / d_kz that is not finite:
 * t = +inf, face = -1, bary = 0.  The result does not depend on the grid, the traversal or the order of the rays: two runs, two grids and a
 * permuted batch agree bit for bit.
 *
 * mnr_mesh_raycast, one thread a ray; with `order` [n] (int64, or NULL) thread i serves ray order[i], as in mnr_mesh_distance.  The walk:
 *   R = 2 max_a max(|o_a|, |origin_a|, |hi_a|);  w = MNR_MESHRAY_MARGIN cell + MNR_MESHRAY_REL R;  wt = min(w |Sz|, FLT_MAX).
 *   Slabs.  c_0 = o_kz + t_min d_kz, c_1 = o_kz + t_max d_kz;  the slabs s (cell index on axis kz) from cell(min(c_0, c_1) - 2 w) to
 *     cell(max(c_0, c_1) + 2 w), none if that range lies outside the grid; in ascending order if d_kz > 0, else descending.
 *   Per slab.  zlo = (origin_kz + float(s) cell) - w,  zhi = (origin_kz + float(s + 1) cell) + w;  ta = (zlo - o_kz) Sz, tb = (zhi - o_kz) Sz,
 *     exchanged if d_kz < 0;  ta = max(ta, t_min) - wt,  tb = min(tb, t_max) + wt.  On each of the axes a = kx, ky:  p = o_a + ta d_a,
 *     p' = o_a + tb d_a (o_a where d_a == 0), the cells cell((min(p, p') - w)) .. cell((max(p, p') + w)), none if that range lies outside
 *     the grid.  Every face of every cell of that rectangle is tested.
 *   Stop after slab s when  best t < tn - 2 wt,  tn = (z - o_kz) Sz with z the plane between slab s and the next one in the ray's
 *     direction.  csrc/meshray.hip argues why no face not yet seen can then have a key at or below the best one.
 *   The slab index advances by one an iteration, at most MNR_MESHDIST_MAX_DIM times.  cell_start entries outside [0, n_pairs], pair_face
 *   entries outside [0, n_faces), face indices outside the vertices and entries of order outside [0, n) are skipped: no access leaves
 *   the inputs.  t_min >= 0 and finite, t_max > t_min.  n == 0 launches nothing; n_pairs == 0: every ray gets the empty result.
 *
 * mnr_raycast_shade, one thread a ray i of n, reads face [n] and bary [n,3] and, of `args`, the mesh (verts, normals, faces), colors or
 * texture + uv, and bg (proj, H, W, near, cull and threshold are not read).  For 0 <= face < n_faces with its three indices inside the
 * vertices, with l = bary: normals [n,3] and rgb [n,3] exactly as mnr_raster_shade writes them from l (the interpolated normal with
 * its two fallbacks; colors, texture or the shaded normal), the same operations in the same order, so equal (face, bary) give equal
 * bits.  Any other ray: normals 0, rgb = bg.
 * ------------------------------------------------------------------------- */
int mnr_mesh_raycast(const mnr_meshdist_args* args, const int64_t* cell_start, const int* pair_face, int64_t n_pairs,
                     const float* origins, const float* directions, const int64_t* order, int64_t n, float t_min, float t_max, int cull,
                     float* t, int* face, float* bary, void* stream);
int mnr_raycast_shade(const mnr_raster_args* args, const int* face, const float* bary, int64_t n, float* normals, float* rgb,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MNERF_H_ */
