"""ctypes binding of include/mnerf.h (cffi is not installed in this image).

The product path has NO CPU fallback: if libmnerf_hip.so is missing or a symbol
declared in the header is absent, importing/using the ops raises.
"""

import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# MNR_LIB_PATH: load another build of the same ABI (same-box A/B of two kernel versions; never a different implementation)
LIB_PATH = os.environ.get('MNR_LIB_PATH') or os.path.join(HERE, 'libmnerf_hip.so')
# The fp32-Dense DEBUG build (multinerf_amd/build.py, csrc/common.h MNR_DENSE_F32): the same kernel sources with float storage and
# plain fp32 Dense layers, loaded on demand for Model(dense_precision='fp32') and active inside `dense_f32()` only.
LIB_F32_PATH = os.path.join(HERE, 'libmnerf_hip_f32.so')
HEADER_PATH = os.path.join(os.path.dirname(HERE), 'include', 'mnerf.h')
# entry points of the layout-specific MFMA files that the fp32 build does not have (the host never calls them in that mode)
F32_ABSENT = ('mnr_mlp_chain_fwd', 'mnr_mlp_chain_fwd_ipe', 'mnr_mlp_chain_bwd')


def describe():
  """Which build is loaded: bench.py records it next to its numbers (an A/B library loaded through MNR_LIB_PATH or a
  build with extra hipcc flags must not pass for the shipped kernels)."""
  stamp = LIB_PATH + '.stamp'
  digest = None
  if os.path.exists(stamp):
    with open(stamp) as f:
      digest = f.read().strip()
  return {'path': os.path.relpath(LIB_PATH, os.path.dirname(HERE)), 'overridden': bool(os.environ.get('MNR_LIB_PATH')),
          'source_digest': digest, 'extra_hipcc_flags': os.environ.get('MNR_EXTRA_HIPCC_FLAGS', '')}

MNR_OK = 0
MNR_ERR_INVALID_ARGUMENT = -1

# enums of mnerf.h
RAYDIST = {None: 0, 'identity': 0, 'reciprocal': 1, 'piecewise': 2, 'log': 3, 'exp': 4, 'sqrt': 5,
           'square': 6}
ACT = {'sigmoid': 0, 'safe_exp': 1, 'softplus': 2, 'exp': 3, 'relu': 4, 'identity': 5}
DATA_LOSS = {'mse': 0, 'charb': 1, 'rawnerf': 2}
NET_ACT = {'softplus': 1, 'silu': 2}          # mnr_act_*_bf16 kinds ('relu' lives in the GEMM epilogues)

c_f32p = C.POINTER(C.c_float)
c_u16p = C.POINTER(C.c_uint16)
c_i32p = C.POINTER(C.c_int32)
vp = C.c_void_p


class ResampleCfg(C.Structure):
  _fields_ = [('n_prev', C.c_int), ('n_samples', C.c_int), ('use_dilation', C.c_int),
              ('dilation', C.c_float), ('domain_lo', C.c_float), ('domain_hi', C.c_float),
              ('anneal', C.c_float), ('resample_padding', C.c_float), ('single_jitter', C.c_int),
              ('max_jitter', C.c_float), ('raydist_fn', C.c_int)]


class IpeCfg(C.Structure):
  _fields_ = [('ray_shape', C.c_int), ('warp_contract', C.c_int), ('disable_integration', C.c_int),
              ('basis_k', C.c_int), ('min_deg', C.c_int), ('max_deg', C.c_int)]


class GemmNTArgs(C.Structure):
  _fields_ = [('A1', vp), ('lda1', C.c_int), ('K1', C.c_int),
              ('A2', vp), ('lda2', C.c_int), ('K2', C.c_int),
              ('Bt', vp), ('ldb', C.c_int),
              ('M', C.c_int64), ('N', C.c_int),
              ('bias', vp), ('n_bias', C.c_int), ('relu', C.c_int),
              ('mask', vp), ('ldmask', C.c_int),
              ('Cb', vp), ('ldcb', C.c_int), ('nb', C.c_int),
              ('Cf', vp), ('ldcf', C.c_int), ('f0', C.c_int), ('nf', C.c_int),
              ('mask_bits_out', vp), ('ld_bits_out', C.c_int),
              ('mask_bits_in', vp), ('ld_bits_in', C.c_int),
              ('bits_row_mod', C.c_int64), ('a1_layout', C.c_int), ('c_layout', C.c_int),
              ('vcol', vp), ('vcol_out', vp), ('vcol_bias', vp), ('walk_descending', C.c_int), ('max_wgs', C.c_int)]


class GemmTNArgs(C.Structure):
  _fields_ = [('A', vp), ('lda', C.c_int), ('K', C.c_int),
              ('B', vp), ('ldb', C.c_int), ('N', C.c_int),
              ('M', C.c_int64), ('C', vp), ('ldc', C.c_int),
              ('k_valid', C.c_int), ('n_valid', C.c_int),
              ('bias_out', vp), ('bias_n_valid', C.c_int), ('gcol', vp), ('gcol_out', vp),
              ('a_layout', C.c_int), ('b_layout', C.c_int), ('m_interleave', C.c_int), ('max_wgs', C.c_int),
              ('rank1_g', vp), ('rank1_w', vp), ('rank1_bits', vp), ('ld_rank1_bits', C.c_int)]


CHAIN_MAX_DEPTH = 8


class MlpChainFwdArgs(C.Structure):
  _fields_ = [('M', C.c_int64), ('W', C.c_int), ('depth', C.c_int),
              ('feat', vp), ('ld_feat', C.c_int), ('K0', C.c_int),
              ('Bt', vp * CHAIN_MAX_DEPTH), ('ldb', C.c_int * CHAIN_MAX_DEPTH), ('bias', vp * CHAIN_MAX_DEPTH),
              ('w_head', vp), ('b_head', vp), ('head_out', vp),
              ('acts', vp * CHAIN_MAX_DEPTH), ('bits', vp * CHAIN_MAX_DEPTH), ('skip_layer', C.c_int)]


CHAIN_IPE_GROUP_COLS = 192          # MNR_CHAIN_IPE_GROUP_COLS


class ChainIpeArgs(C.Structure):
  _fields_ = [('cfg', IpeCfg), ('n', C.c_int), ('tdist', vp), ('origins', vp), ('directions', vp), ('radii', vp),
              ('basis', vp)]


class MlpChainBwdArgs(C.Structure):
  _fields_ = [('M', C.c_int64), ('W', C.c_int), ('depth', C.c_int),
              ('g_head', vp), ('w_head', vp),
              ('bits', vp * CHAIN_MAX_DEPTH), ('Bw', vp * CHAIN_MAX_DEPTH), ('ldb', C.c_int * CHAIN_MAX_DEPTH),
              ('dY', vp * CHAIN_MAX_DEPTH), ('dY_in', vp)]


class PackDesc(C.Structure):
  _fields_ = [('src_off', C.c_int64), ('rows_in', C.c_int), ('cols_out', C.c_int),
              ('dst_off', C.c_int64), ('ld', C.c_int), ('row0', C.c_int), ('col0', C.c_int),
              ('transpose', C.c_int)]


class CompositeCfg(C.Structure):
  _fields_ = [('n', C.c_int), ('opaque_background', C.c_int), ('density_act', C.c_int),
              ('density_bias', C.c_float), ('density_noise_std', C.c_float), ('has_rgb', C.c_int),
              ('rgb_act', C.c_int), ('rgb_premultiplier', C.c_float), ('rgb_bias', C.c_float),
              ('rgb_padding', C.c_float), ('bg_mode', C.c_int), ('bg_value', C.c_float)]


class LevelBwdArgs(C.Structure):
  _fields_ = [('cfg', CompositeCfg), ('B', C.c_int64), ('B_valid', C.c_int64),
              ('raw_density', vp), ('density_noise', vp), ('raw_rgb', vp), ('tdist', vp), ('dirs', vp),
              ('bg', vp), ('exposure_scale', vp), ('weights', vp), ('g_rgb_out', vp), ('g_weights', vp),
              ('g_raw_density', vp), ('g_raw_density_bf16', vp), ('ld_bf16', C.c_int), ('g_raw_rgb', vp),
              ('g_exposure_scale', vp),
              ('data_loss_type', C.c_int), ('charb_padding', C.c_float), ('data_loss_mult', C.c_float),
              ('rgb_out', vp), ('gt', vp), ('lossmult', vp), ('lm_c', C.c_int), ('denom', vp), ('data_stats', vp),
              ('wloss_mode', C.c_int), ('wloss_mult', C.c_float), ('sdist', vp), ('n_ref', C.c_int), ('t_ref', vp),
              ('w_ref', vp), ('wloss_stat', vp), ('g_x', vp)]


class SdistBwdArgs(C.Structure):
  _fields_ = [('B', C.c_int64), ('B_valid', C.c_int64), ('n', C.c_int),
              ('sdist', vp), ('near', vp), ('far', vp), ('raydist_fn', C.c_int),
              ('g_x', vp), ('raw_density', vp), ('density_noise', vp), ('density_noise_std', C.c_float),
              ('density_bias', C.c_float), ('density_act', C.c_int), ('dirs', vp),
              ('g_t0', vp), ('g_t1', vp), ('distortion_mult', C.c_float), ('weights', vp),
              ('g_sdist_in', vp), ('g_sdist', vp)]


class IdeTables(C.Structure):
  _fields_ = [('T', C.c_int), ('lmax', C.c_int), ('m', vp), ('l', vp), ('sigma', vp), ('mat', vp)]


class RobustArgs(C.Structure):
  _fields_ = [('B', C.c_int64), ('B_valid', C.c_int64),
              ('patch_size', C.c_int), ('inner_patch_size', C.c_int), ('filter_size', C.c_int), ('enable', C.c_int),
              ('smoothed_inlier_quantile', C.c_double), ('inner_patch_inlier_quantile', C.c_double),
              ('rgb', vp), ('gt', vp), ('lossmult', vp), ('lm_c', C.c_int), ('loss_threshold', vp), ('denom', vp),
              ('mask', vp), ('lossmult_out', vp), ('err', vp), ('stats', vp), ('mse', vp)]


SSIM_MAX_FILTER = 11               # MNR_SSIM_MAX_FILTER
CC_FEATURES, CC_GRAM_OUT = 10, 65  # MNR_CC_FEATURES, MNR_CC_GRAM_OUT


class SsimArgs(C.Structure):
  _fields_ = [('H', C.c_int), ('W', C.c_int), ('C', C.c_int), ('crop', C.c_int), ('filter_size', C.c_int),
              ('filter_sigma', C.c_double), ('max_val', C.c_double), ('k1', C.c_double), ('k2', C.c_double),
              ('a', vp), ('b', vp), ('map', vp), ('partials', vp), ('out', vp)]


class SqdiffArgs(C.Structure):
  _fields_ = [('H', C.c_int), ('W', C.c_int), ('C', C.c_int), ('crop', C.c_int), ('quantize', C.c_int),
              ('a_f64', C.c_int), ('b_f64', C.c_int), ('a', vp), ('b', vp), ('q_out', vp), ('partials', vp), ('out', vp)]


class CcGramArgs(C.Structure):
  _fields_ = [('N', C.c_int64), ('eps', C.c_double), ('img', vp), ('ref', vp), ('mask0', vp), ('write_mask0', C.c_int),
              ('partials', vp), ('out', vp)]


VIS_MAX_PERCENTILES = 4            # MNR_VIS_MAX_PERCENTILES
VIS_CURVE = {None: 0, 'identity': 0, 'log': 1, 'neg_log': 2, 'ln': 3}
VIS_PREOP = {None: 0, 'none': 0, 'half': 1, 'tanh': 2, 'coord_mod': 3}


class VisCmapArgs(C.Structure):
  _fields_ = [('H', C.c_int), ('W', C.c_int), ('C', C.c_int), ('value', vp), ('lohi', vp), ('curve', C.c_int),
              ('modulus', C.c_double), ('lut', vp), ('n_lut', C.c_int), ('acc', vp), ('dark', C.c_float), ('light', C.c_float),
              ('width', C.c_int), ('out', vp), ('out_u8', vp)]


class VisMatteArgs(C.Structure):
  _fields_ = [('H', C.c_int), ('W', C.c_int), ('C', C.c_int), ('preop', C.c_int), ('x', vp), ('acc', vp), ('origins', vp),
              ('directions', vp), ('distance', vp), ('dark', C.c_float), ('light', C.c_float), ('width', C.c_int), ('out', vp)]


RAW_DTYPE = {'uint16': 0, 'float32': 1}      # mnr_raw_dtype


class RawPostArgs(C.Structure):
  _fields_ = [('P', C.c_int64), ('raw', vp), ('raw_f64', C.c_int), ('camtorgb', C.c_double * 9), ('exposure', C.c_double),
              ('exposure_dev', vp), ('linear_only', C.c_int), ('out_f64', vp), ('out_f32', vp), ('out_u8', vp)]


IMG_DTYPE = {'uint8': 0, 'float32': 1}         # mnr_img_dtype
INGEST_MODE = {'plain': 0, 'white_bg': 1, 'normals': 2}      # mnr_ingest_mode


class MtArgs(C.Structure):
  _fields_ = [('nx', C.c_int), ('ny', C.c_int), ('nz', C.c_int), ('field', vp), ('level', C.c_float), ('origin', C.c_float * 3),
              ('spacing', C.c_float), ('mask', vp), ('counts', vp), ('offsets', vp), ('base', vp), ('verts', vp), ('normals', vp),
              ('n_verts', C.c_int64), ('faces', vp), ('n_faces', C.c_int64)]


TSDF_MAX_FRAMES = 64               # MNR_TSDF_MAX_FRAMES


class TsdfArgs(C.Structure):
  _fields_ = [('nx', C.c_int), ('ny', C.c_int), ('nz', C.c_int), ('origin', C.c_float * 3), ('spacing', C.c_float), ('trunc', C.c_float),
              ('F', C.c_int), ('H', C.c_int), ('W', C.c_int), ('proj', vp), ('depth', vp), ('acc', vp), ('acc_threshold', C.c_float),
              ('rgb', vp), ('tsdf', vp), ('weight', vp), ('color', vp)]


CAM_REC = 28                       # MNR_CAM_REC: floats of a camera record (include/mnerf.h, "The forward camera model")
CAM_MODEL = {'perspective': 0, 'fisheye': 1, 'pano': 2}      # mnr_camtype


class TsdfCamArgs(C.Structure):
  _fields_ = [('nx', C.c_int), ('ny', C.c_int), ('nz', C.c_int), ('origin', C.c_float * 3), ('spacing', C.c_float), ('trunc', C.c_float),
              ('F', C.c_int), ('H', C.c_int), ('W', C.c_int), ('model', C.c_int), ('cameras', vp), ('depth', vp), ('acc', vp),
              ('acc_threshold', C.c_float), ('rgb', vp), ('tsdf', vp), ('weight', vp), ('color', vp)]


QEM_REG = 1e-3                     # MNR_QEM_REG
MESH_CELL_LIMIT = 1 << 21          # MNR_MESH_CELL_LIMIT
MESH_KEY_NONFINITE, MESH_KEY_OUTSIDE = -1, -2


class MeshClusterArgs(C.Structure):
  _fields_ = [('n_clusters', C.c_int64), ('n_verts', C.c_int64), ('n_faces', C.c_int64), ('n_incident', C.c_int64), ('verts', vp),
              ('normals', vp), ('colors', vp), ('faces', vp), ('keys', vp), ('member_start', vp), ('members', vp), ('face_start', vp),
              ('cluster_faces', vp), ('origin', C.c_float * 3), ('cell', C.c_float), ('out_verts', vp), ('out_normals', vp),
              ('out_colors', vp), ('fallback', vp)]


ATLAS_MIN_CELL = 3                 # MNR_ATLAS_MIN_CELL


class AtlasArgs(C.Structure):
  _fields_ = [('verts', vp), ('normals', vp), ('faces', vp), ('n_verts', C.c_int64), ('n_faces', C.c_int64), ('c', C.c_int), ('cols', C.c_int),
              ('W', C.c_int), ('H', C.c_int), ('cov_scale', C.c_float)]


RASTER_CULL = {'none': 0, 'back': 1}           # MNR_RASTER_CULL_*


class RasterArgs(C.Structure):
  _fields_ = [('verts', vp), ('normals', vp), ('faces', vp), ('n_verts', C.c_int64), ('n_faces', C.c_int64), ('proj', C.c_float * 12),
              ('H', C.c_int), ('W', C.c_int), ('near', C.c_float), ('cull', C.c_int), ('threshold', C.c_int64), ('colors', vp),
              ('colors_u8', C.c_int), ('texture', vp), ('texture_u8', C.c_int), ('Ht', C.c_int), ('Wt', C.c_int), ('uv', vp),
              ('bg', C.c_float * 3)]


SHTEX_MAX_DEGREE = 2               # MNR_SHTEX_MAX_DEGREE
SHTEX_MAX_DIRS = 512               # MNR_SHTEX_MAX_DIRS
SH_CONSTANTS = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)   # MNR_SH_C0, C1, C2A, C2B, C2C


class ShtexShadeArgs(C.Structure):
  _fields_ = [('verts', vp), ('faces', vp), ('n_verts', C.c_int64), ('n_faces', C.c_int64), ('face', vp), ('bary', vp), ('H', C.c_int),
              ('W', C.c_int), ('uv', vp), ('sh', vp), ('Ht', C.c_int), ('Wt', C.c_int), ('degree', C.c_int), ('origin', C.c_float * 3)]


MESHDIST_MAX_DIM = 1024            # MNR_MESHDIST_MAX_DIM


ICP_SUMS = 47                      # MNR_ICP_SUMS
CROP_MAX_POLYGON = 4096            # MNR_CROP_MAX_POLYGON


class MeshDistArgs(C.Structure):
  _fields_ = [('verts', vp), ('faces', vp), ('n_verts', C.c_int64), ('n_faces', C.c_int64), ('origin', C.c_float * 3), ('hi', C.c_float * 3),
              ('cell', C.c_float), ('dims', C.c_int * 3)]


class AdamCfg(C.Structure):
  _fields_ = [('lr', C.c_float), ('b1', C.c_float), ('b2', C.c_float), ('eps', C.c_float),
              ('bias_corr1', C.c_float), ('bias_corr2', C.c_float), ('one_minus_b1', C.c_float),
              ('one_minus_b2', C.c_float), ('grad_max_val', C.c_float), ('grad_max_norm', C.c_float)]


i64, i32, f32 = C.c_int64, C.c_int, C.c_float
_PROTOS = {
    'mnr_abi_version': ([], i32),
    'mnr_device_info': ([i32, C.POINTER(i32), C.POINTER(i32), C.c_char_p, i32], i32),
    'mnr_resample_level': ([C.POINTER(ResampleCfg), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_resample_level_bwd': ([C.POINTER(ResampleCfg), i64, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_sorted_interp': ([i64, i32, i32, vp, vp, vp, vp, vp, vp], i32),
    'mnr_max_dilate_weights': ([i64, i32, vp, vp, f32, f32, f32, vp, vp, vp, vp], i32),
    'mnr_cast_rays_ipe': ([C.POINTER(IpeCfg), i64, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp], i32),
    'mnr_cast_rays_ipe_f32': ([C.POINTER(IpeCfg), i64, i32, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_cast_rays_ipe_tangent': ([C.POINTER(IpeCfg), i64, i32, vp, vp, vp, vp, vp, vp, i32, vp], i32),
    'mnr_cast_rays_ipe_bwd': ([C.POINTER(IpeCfg), i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp], i32),
    'mnr_cast_rays_ipe_tangent_bwd': ([C.POINTER(IpeCfg), i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp], i32),
    'mnr_ipe_from_gaussians': ([C.POINTER(IpeCfg), i64, vp, vp, vp, vp, i32, vp, vp, vp, vp], i32),
    'mnr_ipe_from_gaussians_tangent': ([C.POINTER(IpeCfg), i64, vp, vp, vp, vp, i32, vp], i32),
    'mnr_sdist_bwd': ([C.POINTER(SdistBwdArgs), vp], i32),
    'mnr_viewdir_enc_fill': ([i64, i32, vp, i32, vp, i32, i32, i32, vp], i32),
    'mnr_pixels_to_rays': ([i64, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp], i32),
    'mnr_spherical_rays': ([i32, i32, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_glo_fill': ([i64, i32, i32, vp, vp, i32, vp, i32, i32, vp], i32),
    'mnr_glo_bwd': ([i64, i32, i32, vp, vp, vp, i32, vp, vp], i32),
    'mnr_gemm_nt_bf16': ([C.POINTER(GemmNTArgs), vp], i32),
    'mnr_gemm_tn_bf16': ([C.POINTER(GemmTNArgs), vp], i32),
    'mnr_mlp_chain_fwd': ([C.POINTER(MlpChainFwdArgs), vp], i32),
    'mnr_mlp_chain_bwd': ([C.POINTER(MlpChainBwdArgs), vp], i32),
    'mnr_mlp_chain_fwd_ipe': ([C.POINTER(MlpChainFwdArgs), C.POINTER(ChainIpeArgs), vp], i32),
    'mnr_colsum_bf16': ([vp, i32, i64, i32, vp, vp], i32),
    'mnr_pack_weights_bf16': ([vp, vp, i32, i32, vp, vp], i32),
    'mnr_scatter_add_f32': ([vp, i32, i32, i32, i32, i32, vp, i32, vp], i32),
    'mnr_act_fwd_bf16': ([i32, i64, vp, vp, vp], i32),
    'mnr_act_bwd_bf16': ([i32, i64, vp, vp, vp], i32),
    'mnr_act_tangent_fwd_bf16': ([i32, i64, vp, vp, vp, vp], i32),
    'mnr_act_tangent_bwd_bf16': ([i32, i64, vp, vp, vp, vp, vp], i32),
    'mnr_add_noise_bf16': ([i64, i32, vp, i32, vp, f32, vp], i32),
    'mnr_cast_f32_to_bf16': ([vp, i32, i64, i32, vp, i32, i32, vp], i32),
    'mnr_small_head_bwd': ([i64, i32, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, i64, vp, i64, vp], i32),
    'mnr_composite_fwd': ([C.POINTER(CompositeCfg), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_composite_bwd': ([C.POINTER(CompositeCfg), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                           vp, vp, vp], i32),
    'mnr_level_bwd': ([C.POINTER(LevelBwdArgs), vp], i32),
    'mnr_exposure_scale': ([i64, vp, vp, vp, vp, vp], i32),
    'mnr_exposure_scale_bwd': ([i64, vp, vp, vp, vp, vp], i32),
    'mnr_render_extras': ([i64, i32, vp, vp, vp, vp, vp], i32),
    'mnr_ref_head_fwd': ([i64, i32, vp, vp, vp, C.POINTER(IdeTables), i32, i32, f32, vp, i32, i32, i32, vp, vp, vp, vp], i32),
    'mnr_ref_head_bwd': ([i64, i32, vp, vp, vp, C.POINTER(IdeTables), i32, i32, f32, vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, vp, vp],
                         i32),
    'mnr_add_cols_bf16': ([i64, i32, vp, i32, vp, i32, vp, i32, vp], i32),
    'mnr_ref_color_fwd': ([i64, vp, vp, f32, f32, f32, i32, vp, vp], i32),
    'mnr_ref_color_bwd': ([i64, vp, vp, f32, f32, f32, i32, vp, vp, vp, i32, i32, i32, vp], i32),
    'mnr_ref_losses': ([i64, i32, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_weighted_sum': ([i64, i32, i32, vp, vp, vp, vp], i32),
    'mnr_density_normals_fwd': ([i64, vp, vp, vp], i32),
    'mnr_density_normals_bwd': ([i64, vp, vp, vp, vp], i32),
    'mnr_pred_normals_fwd': ([i64, vp, i32, i32, vp, vp], i32),
    'mnr_pred_normals_bwd': ([i64, vp, i32, i32, vp, vp, i32, i32, vp], i32),
    'mnr_lossmult_sum': ([i64, vp, i32, vp, vp], i32),
    'mnr_render_metrics': ([i64, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_data_loss': ([i32, f32, f32, i64, i64, vp, vp, vp, i32, vp, vp, vp, vp], i32),
    'mnr_interlevel_loss': ([f32, i64, i64, i32, vp, vp, i32, vp, vp, vp, vp, vp], i32),
    'mnr_distortion_loss': ([f32, i64, i64, i32, vp, vp, vp, vp, vp], i32),
    'mnr_lossfun_outer': ([i64, i32, vp, vp, i32, vp, vp, vp, vp], i32),
    'mnr_lossfun_distortion': ([i64, i32, vp, vp, vp, vp], i32),
    'mnr_robustnerf_mask': ([C.POINTER(RobustArgs), vp], i32),
    'mnr_quantile': ([i64, vp, C.c_double, vp, vp], i32),
    'mnr_ssim_partials': ([i32, i32, i32, i32, i32], i32),
    'mnr_ssim': ([C.POINTER(SsimArgs), vp], i32),
    'mnr_image_sqdiff_partials': ([i64], i32),
    'mnr_image_sqdiff': ([C.POINTER(SqdiffArgs), vp], i32),
    'mnr_cc_gram_partials': ([i64], i32),
    'mnr_cc_gram': ([C.POINTER(CcGramArgs), vp], i32),
    'mnr_cc_apply': ([i64, vp, C.POINTER(C.c_double), vp, vp], i32),
    'mnr_weighted_percentile_partials': ([i64], i32),
    'mnr_weighted_percentile': ([i64, vp, vp, i64, vp, i32, C.POINTER(C.c_double), vp, vp, vp], i32),
    'mnr_vis_cmap': ([C.POINTER(VisCmapArgs), vp], i32),
    'mnr_vis_matte': ([C.POINTER(VisMatteArgs), vp], i32),
    'mnr_raw_demosaic': ([i32, i32, i32, i32, vp, vp, vp, C.c_double, i32, vp, vp], i32),
    'mnr_raw_postprocess': ([C.POINTER(RawPostArgs), vp], i32),
    'mnr_quantile_f64_workspace': ([i64], i64),
    'mnr_quantile_f64': ([i64, vp, C.c_double, vp, vp, vp], i32),
    'mnr_affine_sums_partials': ([i64], i32),
    'mnr_affine_sums': ([i64, vp, vp, vp, vp, vp], i32),
    'mnr_affine_apply': ([i64, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, vp], i32),
    'mnr_image_ingest': ([i32, i32, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp], i32),
    'mnr_mt_workgroups': ([i64], i64),
    'mnr_mt_classify': ([C.POINTER(MtArgs), vp], i32),
    'mnr_mt_emit_vertices': ([C.POINTER(MtArgs), vp], i32),
    'mnr_mt_emit_faces': ([C.POINTER(MtArgs), vp], i32),
    'mnr_tsdf_integrate': ([C.POINTER(TsdfArgs), vp], i32),
    'mnr_tsdf_integrate_cam': ([C.POINTER(TsdfCamArgs), vp], i32),
    'mnr_project_points': ([i64, vp, C.POINTER(C.c_float), vp, vp, vp, vp], i32),
    'mnr_mt_vertex_valid': ([C.POINTER(MtArgs), vp, vp, vp], i32),
    'mnr_mesh_cc_init': ([i64, vp, vp], i32),
    'mnr_mesh_cc_sweep': ([vp, i64, i64, vp, vp, vp], i32),
    'mnr_mesh_cluster_keys': ([vp, i64, C.POINTER(f32), f32, vp, vp], i32),
    'mnr_mesh_cluster_faces': ([vp, i64, vp, i64, i64, vp, vp, vp, vp, vp], i32),
    'mnr_mesh_cluster_solve': ([C.POINTER(MeshClusterArgs), vp], i32),
    'mnr_atlas_samples': ([C.POINTER(AtlasArgs), i64, i64, vp, vp, vp, vp, vp, vp], i32),
    'mnr_atlas_store': ([C.POINTER(AtlasArgs), i64, i64, vp, vp, vp, vp, vp, vp], i32),
    'mnr_atlas_uvs': ([C.POINTER(AtlasArgs), vp, vp], i32),
    'mnr_raster_visibility': ([C.POINTER(RasterArgs), vp, vp, vp, vp], i32),
    'mnr_raster_shade': ([C.POINTER(RasterArgs), vp, vp, vp, vp, vp, vp, vp, vp], i32),
    'mnr_shtex_weights': ([vp, i64, vp, i64, vp, vp], i32),
    'mnr_shtex_fit': ([vp, vp, i64, i32, vp, vp, i64, C.c_double, vp, vp], i32),
    'mnr_shtex_shade': ([C.POINTER(ShtexShadeArgs), vp, vp], i32),
    'mnr_mesh_grid_count': ([C.POINTER(MeshDistArgs), vp, vp], i32),
    'mnr_mesh_grid_fill': ([C.POINTER(MeshDistArgs), vp, i64, vp, vp, vp], i32),
    'mnr_mesh_distance': ([C.POINTER(MeshDistArgs), vp, vp, i64, vp, vp, i64, f32, vp, vp, vp, vp], i32),
    'mnr_mesh_face_areas': ([vp, i64, vp, i64, vp, vp], i32),
    'mnr_mesh_sample': ([vp, i64, vp, i64, vp, i64, C.c_uint32, vp, vp, vp], i32),
    'mnr_mesh_closest': ([vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, vp], i32),
    'mnr_mesh_face_normals': ([vp, i64, vp, i64, vp, vp], i32),
    'mnr_icp_sums_partials': ([i64], i32),
    'mnr_icp_sums': ([i64, vp, vp, vp, vp, C.POINTER(C.c_double), vp, vp, vp], i32),
    'mnr_crop_polygon': ([vp, i64, vp, i32, i32, C.c_double, C.c_double, vp, vp], i32),
    'mnr_mesh_raycast': ([C.POINTER(MeshDistArgs), vp, vp, i64, vp, vp, vp, i64, f32, f32, i32, vp, vp, vp, vp], i32),
    'mnr_raycast_shade': ([C.POINTER(RasterArgs), vp, vp, i64, vp, vp, vp], i32),
    'mnr_weight_decay': ([vp, i64, i64, f32, vp, vp, vp, vp], i32),
    'mnr_grad_sqnorm': ([vp, i64, i64, f32, vp, vp], i32),
    'mnr_clip_adam': ([C.POINTER(AdamCfg), i64, i64, vp, vp, vp, vp, vp, vp], i32),
}

# include/mnerf_debug.h: development / test hooks (process-global A/B switches, small-grid test hooks, timelines).  The
# package never calls them; tests/ and tools/ reach them through debug().
_DEBUG_PROTOS = {
    'mnr_debug_gemm_timeline': ([vp], i32),
    'mnr_gemm_nt_set_persistent': ([i32], i32),
    'mnr_level_bwd_set_quad': ([i32], i32),
    'mnr_gemm_nt_set_pipelined': ([i32], i32),
    'mnr_gemm_nt_set_wres': ([i32], i32),
    'mnr_gemm_nt_panel_set_max_wgs': ([i32], i32),
    'mnr_debug_chain_timeline': ([vp], i32),
    'mnr_mlp_chain_set_deferred': ([i32], i32),
    'mnr_mlp_chain_set_max_wgs': ([i32], i32),
}

_lib = None


def header_symbols(path=None):
  """Every function name include/mnerf.h (or the header at `path`) declares."""
  with open(path or HEADER_PATH) as f:
    text = f.read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(mnr_[a-z0-9_]+)\s*\(', text)))


def _bind(path, absent=()):
  if not os.path.exists(path):
    raise RuntimeError(
        f'{path} is missing: the HIP extension has not been built. Run '
        '`python -m multinerf_amd.build` (needs hipcc, ROCm >= 7.0). There is no CPU fallback.')
  # torch must load ITS HIP runtime first: libmnerf_hip.so then binds to that same libamdhip64
  # instead of pulling a second copy from /opt/rocm (two runtimes in one process cannot share the device).
  import torch  # noqa: F401
  lib = C.CDLL(path)
  lib.mnr_last_error.restype = C.c_char_p
  lib.mnr_last_error.argtypes = []
  for name, (argtypes, restype) in _PROTOS.items():
    if name in absent:
      continue
    fn = getattr(lib, name)      # AttributeError if the symbol is missing
    fn.argtypes = argtypes
    fn.restype = restype
  return lib


_lib_f32 = None
_f32_depth = 0                    # > 0: inside dense_f32(): load() hands out the fp32-Dense debug build


def load():
  """Load libmnerf_hip.so (inside `dense_f32()`: libmnerf_hip_f32.so); raises (never falls back) when it is unavailable."""
  global _lib, _lib_f32
  if _f32_depth > 0:
    if _lib_f32 is None:
      _lib_f32 = _bind(LIB_F32_PATH, F32_ABSENT)
    return _lib_f32
  if _lib is None:
    _lib = _bind(LIB_PATH)
  return _lib


def f32_active():
  return _f32_depth > 0


class dense_f32:
  """Context: the C-ABI calls inside go to the fp32-Dense debug build, and what include/mnerf.h calls a bf16 matrix (uint16_t*)
  is a float matrix.  Re-entrant; `on=False` makes it a no-op (so that callers can write `with model.library():`)."""

  def __init__(self, on=True):
    self.on = bool(on)

  def __enter__(self):
    global _f32_depth
    if self.on:
      _f32_depth += 1
    return self

  def __exit__(self, *exc):
    global _f32_depth
    if self.on:
      _f32_depth -= 1
    return False


DEBUG_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), 'mnerf_debug.h')


def debug(handle=None):
  """The loaded library with the hooks of include/mnerf_debug.h bound (tests / tools only)."""
  lib = handle if handle is not None else load()
  for name, (argtypes, restype) in _DEBUG_PROTOS.items():
    fn = getattr(lib, name)
    fn.argtypes = argtypes
    fn.restype = restype
  return lib


def check(status):
  if status == MNR_OK:
    return
  msg = load().mnr_last_error().decode()
  if status == MNR_ERR_INVALID_ARGUMENT:
    raise ValueError(msg)
  raise RuntimeError(f'libmnerf_hip status {status}: {msg}')
