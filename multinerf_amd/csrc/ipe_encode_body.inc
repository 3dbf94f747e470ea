// Phases 2 and 3 of the IPE featurisation kernels: the encode loop, the padding loop and the 16-byte write-out.
// cast_rays_ipe_kernel (features.hip) and ipe_from_gaussians_kernel (gaussians.hip) include this file textually behind the
// __syncthreads() that ends their phase 1, as the last statements of the kernel function, with floating-point contraction
// off.  (Textual, not a __forceinline__ function: that keeps both kernels' device code what profiles/r6_validated_isa.json pins.)
// In scope:
//   template <bool OUT_F32, bool TANGENT>   fp32 rows without padding / three tangent rows per sample ([c][sample][ld])
//   FE_THREADS                              the block size (ipe_math.h)
//   mnr_ipe_cfg c; int K, L, nfeat          basis directions, degrees, 2 K L
//   int64_t total, s0; int ns, spb          samples in all, the block's first sample, its count (<= spb), samples per block
//   int pitch                               bytes between staged rows in LDS (fe_block_geometry, ipe_math.h)
//   FeSample* gs; FeTangent* gt; float* bs  LDS: the block's Gaussians, their tangents (TANGENT only), the basis [K][3]
//   char* rows                              LDS: the staged rows [spb][pitch] (x 3 if TANGENT)
//   void* feat_out; int ld_feat             the rows in HBM, and their length in elements (bf16 rows)
  const int row_elems = OUT_F32 ? nfeat : ld_feat;
  // `pitch`: bytes between staged rows in LDS (row bytes + padding: with 1-KiB rows every sample of a wave hits the same banks).
  // The kernel streams its feature rows out at 3.0-3.9 TB/s (1 GB per 64-sample proposal level in 0.27-0.36 ms).  That is NOT the
  // write rate HBM sustains (a plain fill writes 6.9 TB/s, profiles/r5k_write_rate.txt): without its write-out the kernel takes 246 of
  // its 357 us, without the encoding loop 191 (profiles/r5m_ipe_probe.txt): the two phases of a block barely overlap with the
  // other blocks of its CU.  Round 2 cut the loop from ≈470 to ≈340 instructions per (sample, direction) without changing the
  // time; round 5's two-directions-per-thread loop on v_pk_mul_f32 (1.7x fewer instructions, same bits) was 5-9 % SLOWER
  // (profiles/r5n_probe.txt) and is not here.  The inner loop is short rather than clever:
  // an anchor every 4th degree = one sin / cos of the wrapped argument (math.safe_sin's wrap at float32(100 pi),
  // math.py:26-28; fe_sincos_wrapped) and one hardware exp2 for the attenuation; the 3 degrees behind it by the double-angle
  // recurrence (sin 2x = 2 sin x cos x, cos 2x = 1 - 2 sin^2 x; cf. stable_pos_enc in the reference's tests/coord_test.py:34-43)
  // and by att(l+1) = att(l)^4 (exp(-v 4^l / 2): two squarings): at most 3 steps of a ~1e-7 error, each at most x4.
  // cos is the reference's sin(x + pi/2).  sin and cos feature of a (degree, direction) leave as one packed bf16 pair.
  // TANGENT: three rows per sample (d/d mean_x, d/d mean_y, d/d mean_z), staged as [c][sample][ld].
  const float inv_k = 1.0f / (float)K;
#if defined(FE_DBG) && FE_DBG == 1                      // timing probe (tools/ipe_probe.py): no encoding (rows are whatever LDS holds)
  for (int pair = threadIdx.x; pair < 0; pair += FE_THREADS) {
#else
  for (int pair = threadIdx.x; pair < ns * K; pair += FE_THREADS) {
#endif
    const int si = (int)(((float)pair + 0.5f) * inv_k);       // pair / K, exact for pair < 2^20
    const int k = pair - si * K;
    const FeSample g = gs[si];
    const float px = bs[k * 3 + 0], py = bs[k * 3 + 1], pz = bs[k * 3 + 2];
    // coord.py:131-132: mean . p_k ; p_k^T cov p_k.  (fe_project, ipe_math.h, written out: through the helper hipcc orders
    // cast_rays_ipe_kernel<false, true> differently, and the pinned device code is the validated one.)
    const float lm = g.mean[0] * px + g.mean[1] * py + g.mean[2] * pz;
    const float cx = g.cov[0] * px + g.cov[1] * py + g.cov[2] * pz;
    const float cy = g.cov[1] * px + g.cov[3] * py + g.cov[4] * pz;
    const float cz = g.cov[2] * px + g.cov[4] * py + g.cov[5] * pz;
    const float lv = px * cx + py * cy + pz * cz;
    const float vscale = -0.5f * 1.44269504088896340736f * lv;       // exp(-v/2) = exp2(vscale * 4^deg)
    char* rowp = rows + (size_t)si * pitch + (size_t)k * (OUT_F32 ? 4 : (int)sizeof(bf16));       // column k of the sample's row (row 0 of 3 if TANGENT)
    const int half = K * L * (OUT_F32 ? 4 : (int)sizeof(bf16));                      // byte offset of the cos half of the row
    const int lstep = K * (OUT_F32 ? 4 : (int)sizeof(bf16));
    float sc = ldexpf(1.0f, c.min_deg);                              // 2^deg, exact
    float sn = 0.0f, cs = 1.0f, att = 1.0f;
    float dlm[3] = {px, py, pz}, dlv[3] = {0.0f, 0.0f, 0.0f};
    if (TANGENT) {
      const FeTangent& T = gt[si];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) fe_project_tangent(T, cc, px, py, pz, &dlm[cc], &dlv[cc]);
    }
    for (int l = 0; l < L; ++l) {
      if ((l & 3) == 0) fe_anchor(lm, vscale, sc, &sn, &cs, &att);
      const float fs = att * sn;
      const float fc = att * cs;
      if (TANGENT) {
        // d/d mean_c of att sin(lm 2^l) = att 2^l cos(.) dlm_c - 1/2 4^l att sin(.) dlv_c;  of att cos(.): -att 2^l sin(.) dlm_c
        // - 1/2 4^l att cos(.) dlv_c, with dlm_c = p_k . dz[c], dlv_c = p_k^T dC[c] p_k (no warp: dlm_c = p_k[c], dlv_c = 0:
        // the variance does not depend on the mean).
        const float hv = -0.5f * sc * sc;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          char* rp = rowp + (size_t)cc * spb * pitch;
          *(bf16*)rp = (bf16)(fc * sc * dlm[cc] + hv * fs * dlv[cc]);
          *(bf16*)(rp + half) = (bf16)(-fs * sc * dlm[cc] + hv * fc * dlv[cc]);
        }
      } else if (OUT_F32) {
        *(float*)rowp = fs;
        *(float*)(rowp + half) = fc;
      } else {
        const f32x2 pr = {fs, fc};
        const bf16x2 pb = __builtin_convertvector(pr, bf16x2);       // one v_cvt_pk_bf16_f32
#if defined(FE_DBG) && FE_DBG == 4                      // timing probe: one LDS store per (sample, direction) instead of 2 L
        if (l == L - 1) *(bf16x2*)(rows + (size_t)si * pitch + (size_t)k * 4) = pb;
#else
        *(bf16*)rowp = pb[0];
        *(bf16*)(rowp + half) = pb[1];
#endif
      }
      rowp += lstep;
      fe_degree_step(&sn, &cs, &att, &sc);
    }
  }
  if (!OUT_F32) {
    // zero the padding columns [nfeat, ld)
    const int pad = ld_feat - nfeat;
    const int nrows = TANGENT ? 3 * spb : ns;
    for (int e = threadIdx.x; e < nrows * pad; e += FE_THREADS) {
      const int si = e / pad, cidx = nfeat + e % pad;
      ((bf16*)(rows + (size_t)si * pitch))[cidx] = (bf16)0.0f;
    }
  }
  __syncthreads();
  // Coalesced write-out: the block's rows are contiguous in HBM (16 B per lane); in LDS they are `pitch` apart.
  const int row_bytes = row_elems * (OUT_F32 ? 4 : (int)sizeof(bf16));
  const int cpr = row_bytes >> 4;                         // 16-B chunks per row (row_bytes is a multiple of 16)
  for (int cc = 0; cc < (TANGENT ? 3 : 1); ++cc) {
    char* dst = (char*)feat_out + ((size_t)cc * total + s0) * row_bytes;
    const char* src = rows + (size_t)cc * spb * pitch;
#if defined(FE_DBG) && FE_DBG == 2                      // timing probe: no write-out (one chunk per block keeps the encoding alive)
    for (int ch = threadIdx.x; ch < 1; ch += FE_THREADS) {
#else
    for (int ch = threadIdx.x; ch < ns * cpr; ch += FE_THREADS) {
#endif
      const int r = ch / cpr, o = (ch - r * cpr) << 4;
      *(uint4*)(dst + (size_t)r * row_bytes + o) = *(const uint4*)(src + (size_t)r * pitch + o);
    }
  }
