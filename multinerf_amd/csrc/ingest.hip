// Image ingest on device (gfx950): decoded pixels as the files hold them (uint8, or float32 for TIFF inputs) -> the float32
// tensors a dataset keeps in HBM.  What the reference's loaders do per pixel on the host, in its float32 order:
//
//   image.downsample's block mean        m = float(S) / float(n n) with S the exact integer sum (uint8), or the float64 sum of
//                                        the block added row by row (dy outer, dx inner), divided by n n in float64 and
//                                        rounded once (float32) -- the rule of mnr_raw_demosaic's downsample;
//   `/ 255.`                             v = m / 255.f (uint8), v = m (float32);
//   `rgb * alpha + (1. - alpha)`         MNR_INGEST_WHITE_BG: product, difference and sum each rounded on their own;
//   `x * 2. / 255. - 1.`                 MNR_INGEST_NORMALS.
//
// Rounding: floating-point contraction is switched OFF for this whole file by the pragma below (the composite `v a + (1 - a)`
// would otherwise become one fused multiply-add and lose bit-equality with the host expression); divisions are the
// correctly rounded IEEE ones hipcc emits by default.
//
// All of it is bound by memory; every source byte is read once and no atomics are used, so two runs agree bit for bit.
//   n = 1, every channel kept, no alpha: the image is a flat array.  A lane takes 4 consecutive elements (one dword of
//          bytes, or one 16-byte load of floats) and writes one 16-byte store: both sides contiguous over the wave.
//   n = 1, otherwise: a lane per pixel, C consecutive elements in (one dword for C = 4 bytes), C_out consecutive floats out.
//   n > 1: a workgroup owns one output row of a strip of `tw` output pixels.  Per source row its lanes copy the strip's
//          tw n C consecutive elements into LDS (dword loads between the strip's unaligned ends), then a lane per output
//          pixel adds its n C values of that row from LDS into registers; after the n rows it finishes and stores the pixel.
// Offsets are 64-bit throughout.
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

#define IG_THREADS 256
#define IG_LDS_ELEMS 4096          // elements of one staged source-row strip (4 KiB of bytes, 16 KiB of floats)

struct ig_args {
  int H, W, C_out, n, mode;
  int tw, tiles_x;                 // n > 1: output pixels per workgroup, workgroups per output row
  int aligned;                     // src is 4-byte aligned (uint8, C = 4: a pixel is one dword)
  int64_t count;                   // flat kernel: elements; pixel kernel: pixels; strip kernel: workgroups
  const void* src;
  float* out;
  float* alpha;
};

// one pixel from its block means m[0..C): what is stored to o[0..C_out) and *alpha
template <int C, bool U8>
__device__ __forceinline__ void ig_finish(const float* m, int mode, int C_out, float* o, float* alpha) {
  if (mode == MNR_INGEST_NORMALS) {                        // (uint8, C >= 3: checked by the launcher)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c < C) o[c] = m[c] * 2.f / 255.f - 1.f;
    }
    return;
  }
  float v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = U8 ? m[c] / 255.f : m[c];
  if (mode == MNR_INGEST_WHITE_BG) {                       // (C == 4)
    const float a = v[C - 1], rest = 1.f - a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c < C) o[c] = v[c] * a + rest;
    }
    if (alpha) *alpha = a;
    return;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (c < C_out) o[c] = v[c];
  }
}

// n = 1, C_out = C, PLAIN or NORMALS (C = 3): elementwise; src 4-byte (uint8) / 16-byte (float32) and out 16-byte aligned
template <bool U8>
__global__ __launch_bounds__(IG_THREADS) void ingest_flat_kernel(ig_args a) {
  const int64_t i = ((int64_t)blockIdx.x * IG_THREADS + threadIdx.x) * 4;
  if (i >= a.count) return;
  const bool normals = a.mode == MNR_INGEST_NORMALS;
  float m[4];
  const int valid = a.count - i >= 4 ? 4 : (int)(a.count - i);
  if (valid == 4) {
    if (U8) {
      const unsigned w = *(const unsigned*)((const unsigned char*)a.src + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = (float)((w >> (8 * k)) & 255u);
    } else {
      const f32x4 w = *(const f32x4*)((const float*)a.src + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = w[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m[k] = 0.f;
      if (k < valid) m[k] = U8 ? (float)((const unsigned char*)a.src)[i + k] : ((const float*)a.src)[i + k];
    }
  }
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = normals ? m[k] * 2.f / 255.f - 1.f : (U8 ? m[k] / 255.f : m[k]);
  if (valid == 4) {
    *(f32x4*)(a.out + i) = r;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < valid) a.out[i + k] = r[k];
    }
  }
}

// n = 1, the other cases: a lane per pixel
template <int C, bool U8>
__global__ __launch_bounds__(IG_THREADS) void ingest_pixel_kernel(ig_args a) {
  const int64_t p = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x;
  if (p >= a.count) return;
  float m[C];
  if (U8) {
    const unsigned char* s = (const unsigned char*)a.src + p * C;
    if (C == 4 && a.aligned) {
      const unsigned w = *(const unsigned*)s;
#pragma unroll
      for (int c = 0; c < C; ++c) m[c] = (float)((w >> (8 * c)) & 255u);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) m[c] = (float)s[c];
    }
  } else {
    const float* s = (const float*)a.src + p * C;
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = s[c];
  }
  float o[4];
  ig_finish<C, U8>(m, a.mode, a.C_out, o, a.alpha ? a.alpha + p : nullptr);
  float* dst = a.out + p * a.C_out;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (c < a.C_out) dst[c] = o[c];
  }
}

// n > 1: see the head of the file.  IG_PIX<C> output pixels per lane at most, so that a lane holds 8 sums or fewer.
template <int C>
struct ig_pix {
  static constexpr int value = 8 / C;
};

template <int C, bool U8>
__global__ __launch_bounds__(IG_THREADS) void ingest_strip_kernel(ig_args a) {
  typedef typename std::conditional<U8, unsigned char, float>::type src_t;
  typedef typename std::conditional<U8, unsigned, double>::type acc_t;
  constexpr int J = ig_pix<C>::value;
  __shared__ __attribute__((aligned(16))) src_t l_row[IG_LDS_ELEMS + 4];
  const int t = threadIdx.x, n = a.n;
  const int Ho = a.H / n, Wo = a.W / n;
  const int64_t b = blockIdx.x;
  const int tile = (int)(b % a.tiles_x);
  const int64_t rest = b / a.tiles_x;
  const int oy = (int)(rest % Ho);
  const int64_t img = rest / Ho;
  const int ox0 = tile * a.tw;
  const int tw = min(a.tw, Wo - ox0);
  const int cnt = tw * n * C;                              // elements of the strip in one source row, <= IG_LDS_ELEMS
  acc_t acc[J][C];
#pragma unroll
  for (int j = 0; j < J; ++j) {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[j][c] = 0;
  }
  for (int r = 0; r < n; ++r) {
    const src_t* s = (const src_t*)a.src + ((img * a.H + ((int64_t)oy * n + r)) * a.W + (int64_t)ox0 * n) * C;
    int shift = 0;                                         // LDS index of the strip's first element
    if (U8) {
      // bytes up to the first 4-byte boundary, whole dwords, the bytes after the last one; the LDS copy keeps the
      // source's alignment so that the dwords are stored whole
      const unsigned char* sb = (const unsigned char*)s;
      unsigned char* lb = (unsigned char*)l_row;
      shift = (int)((size_t)sb & 3);
      int head = (4 - shift) & 3;
      head = head < cnt ? head : cnt;
      const int dwords = (cnt - head) >> 2, tail0 = head + 4 * dwords;
      if (t < head) lb[shift + t] = sb[t];
      for (int i = t; i < dwords; i += IG_THREADS) *(unsigned*)(lb + shift + head + 4 * i) = *(const unsigned*)(sb + head + 4 * i);
      if (t < cnt - tail0) lb[shift + tail0 + t] = sb[tail0 + t];
    } else {
      for (int i = t; i < cnt; i += IG_THREADS) l_row[i] = s[i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int p = t + j * IG_THREADS;
      if (p < tw) {
        const src_t* lp = l_row + shift + p * n * C;
        for (int dx = 0; dx < n; ++dx) {
#pragma unroll
          for (int c = 0; c < C; ++c) acc[j][c] += (acc_t)lp[dx * C + c];
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int p = t + j * IG_THREADS;
    if (p >= tw) continue;
    float m[C], o[4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (U8) {
        m[c] = (float)acc[j][c] / (float)(n * n);
      } else {
        m[c] = (float)((double)acc[j][c] / ((double)n * (double)n));
      }
    }
    const int64_t px = (img * Ho + oy) * Wo + ox0 + p;
    ig_finish<C, U8>(m, a.mode, a.C_out, o, a.alpha ? a.alpha + px : nullptr);
    float* dst = a.out + px * a.C_out;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c < a.C_out) dst[c] = o[c];
    }
  }
}

template <int C, bool U8>
static void ig_launch(const ig_args& a, bool strip, hipStream_t stream) {
  const dim3 block(IG_THREADS);
  if (strip) {
    hipLaunchKernelGGL((ingest_strip_kernel<C, U8>), dim3((unsigned)a.count), block, 0, stream, a);
  } else {
    hipLaunchKernelGGL((ingest_pixel_kernel<C, U8>), dim3((unsigned)((a.count + IG_THREADS - 1) / IG_THREADS)), block, 0, stream, a);
  }
}

template <bool U8>
static void ig_launch_c(int C, const ig_args& a, bool strip, hipStream_t stream) {
  switch (C) {
    case 1: ig_launch<1, U8>(a, strip, stream); break;
    case 2: ig_launch<2, U8>(a, strip, stream); break;
    case 3: ig_launch<3, U8>(a, strip, stream); break;
    default: ig_launch<4, U8>(a, strip, stream); break;
  }
}

extern "C" int mnr_image_ingest(int N, int H, int W, int C, int dtype, const void* src, int n_downsample, int mode, int C_out,
                                float* out, float* alpha, void* stream) {
  const int n = n_downsample;
  MNR_CHECK_ARG(dtype == MNR_IMG_U8 || dtype == MNR_IMG_F32, "mnr_image_ingest: dtype %d is neither MNR_IMG_U8 nor MNR_IMG_F32", dtype);
  MNR_CHECK_ARG(mode == MNR_INGEST_PLAIN || mode == MNR_INGEST_WHITE_BG || mode == MNR_INGEST_NORMALS,
                "mnr_image_ingest: mode %d is not a mnr_ingest_mode", mode);
  MNR_CHECK_ARG(C >= 1 && C <= 4, "mnr_image_ingest: needs 1 <= C <= 4 channels, got %d", C);
  MNR_CHECK_ARG(C_out >= 1 && C_out <= C, "mnr_image_ingest: needs 1 <= C_out <= C = %d, got %d", C, C_out);
  MNR_CHECK_ARG(N >= 0 && H >= 1 && W >= 1, "mnr_image_ingest: needs N >= 0 images of H, W >= 1, got [%d, %d, %d]", N, H, W);
  MNR_CHECK_ARG(n >= 1 && H % n == 0 && W % n == 0, "mnr_image_ingest: n_downsample = %d must divide the image shape [%d, %d]", n, H, W);
  MNR_CHECK_ARG(dtype != MNR_IMG_U8 || n <= 256, "mnr_image_ingest: n_downsample = %d > 256 (the uint8 block sum must stay exact in float32)", n);
  MNR_CHECK_ARG((int64_t)n * C <= IG_LDS_ELEMS, "mnr_image_ingest: n_downsample * C = %lld exceeds the %d values of a staged row",
                (long long)n * C, IG_LDS_ELEMS);
  if (mode == MNR_INGEST_WHITE_BG) {
    MNR_CHECK_ARG(C == 4 && C_out == 3, "mnr_image_ingest: MNR_INGEST_WHITE_BG needs C = 4 and C_out = 3, got %d and %d", C, C_out);
  } else {
    MNR_CHECK_ARG(alpha == nullptr, "mnr_image_ingest: alpha is written by MNR_INGEST_WHITE_BG only");
  }
  if (mode == MNR_INGEST_NORMALS) {
    MNR_CHECK_ARG(dtype == MNR_IMG_U8, "mnr_image_ingest: MNR_INGEST_NORMALS needs uint8 input");
    MNR_CHECK_ARG(C >= 3 && C_out == 3, "mnr_image_ingest: MNR_INGEST_NORMALS needs C >= 3 and C_out = 3, got %d and %d", C, C_out);
  }
  if (N == 0) return MNR_OK;
  MNR_CHECK_ARG(src && out, "mnr_image_ingest: needs a source and an output");
  const bool u8 = dtype == MNR_IMG_U8;
  MNR_CHECK_ARG(u8 || ((size_t)src & 3) == 0, "mnr_image_ingest: a float32 source must be aligned to 4 bytes");
  MNR_CHECK_ARG(((size_t)out & 3) == 0 && ((size_t)alpha & 3) == 0, "mnr_image_ingest: out and alpha must be aligned to 4 bytes");
  const int Ho = H / n, Wo = W / n;
  ig_args a;
  a.H = H;
  a.W = W;
  a.C_out = C_out;
  a.n = n;
  a.mode = mode;
  a.tw = a.tiles_x = 0;
  a.aligned = ((size_t)src & 3) == 0;
  a.src = src;
  a.out = out;
  a.alpha = alpha;
  const int64_t pixels = (int64_t)N * Ho * Wo;
  if (n == 1) {
    const bool flat = C_out == C && mode != MNR_INGEST_WHITE_BG && ((size_t)src & (u8 ? 3 : 15)) == 0 && ((size_t)out & 15) == 0;
    a.count = flat ? pixels * C : pixels;
    MNR_CHECK_ARG((a.count + IG_THREADS - 1) / IG_THREADS < (1ll << 31), "mnr_image_ingest: image stack too large for one launch");
    if (flat) {
      const dim3 grid((unsigned)(((a.count + 3) / 4 + IG_THREADS - 1) / IG_THREADS)), block(IG_THREADS);
      if (u8) {
        hipLaunchKernelGGL(ingest_flat_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
      } else {
        hipLaunchKernelGGL(ingest_flat_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
      }
    } else if (u8) {
      ig_launch_c<true>(C, a, false, (hipStream_t)stream);
    } else {
      ig_launch_c<false>(C, a, false, (hipStream_t)stream);
    }
  } else {
    int tw = IG_LDS_ELEMS / (n * C);
    tw = tw < Wo ? tw : Wo;
    tw = tw < IG_THREADS * (8 / C) ? tw : IG_THREADS * (8 / C);
    a.tw = tw;
    a.tiles_x = mnr_cdiv(Wo, tw);
    a.count = (int64_t)a.tiles_x * Ho * N;
    MNR_CHECK_ARG(a.count < (1ll << 31), "mnr_image_ingest: image stack too large for one launch");
    if (u8) {
      ig_launch_c<true>(C, a, true, (hipStream_t)stream);
    } else {
      ig_launch_c<false>(C, a, true, (hipStream_t)stream);
    }
  }
  MNR_CHECK_LAUNCH();
  return MNR_OK;
}
