// thip_encode_skip.h -- the rate-distortion skip decision of inter frames (TH_ENCCTL_THIP_SET_RD_SKIP; the rule is stated in
// theoraenc_hip.h, "Skip decision"): the skip forms of the two block-qi kernels of an inter frame, one body (enc_fq_skip) over the
// pieces of enc_fq_bqi (thip_encode_bqi.h): enc_stage_rows, fdct4_lds, quantize4_lds, bqi_ac_bits, bqi_sum4, bqi_choose, wave_blocks_out_of.
// With block qi off the same kernels run with a one-entry qi list.  What the body adds to enc_fq_bqi's:
//   SSD     while a lane stages its two rows of the residual it also sums the squared differences of the source against PREV at the
//           block's own position (two dword reads a row where the plane's base and pitch allow, else eight bytes); two shuffles add
//           the four lanes' sums;
//   D_code  the squared error of the chosen levels at z >= 1 (enc_fq_bqi's D_k) plus that of the DC at qis[0] (the lane that holds it
//           keeps it from the quantiser's hook of the first qi);
//   the test  D_skip <= D_code + lambda_b R_k leaves the block uncoded, where the rules of enc_fq_tail would have coded it -- never a
//           luma block of an INTER_MV_FOUR macro block;
//   chroma  a chroma block reads its macro block's four luma cmap entries: when none is coded the macro block writes no mode and the
//           block is predicted, transformed and classed as an INTER_NOMV block whatever the word says.
// Hence two launches a frame over ranges of the coded order: the luma blocks, then the chroma blocks (skip_launch below, which
// th_encode_* and thip_enc_skip_stage both call).  No atomics but dclast's, nothing that depends on the order of waves.
#pragma once
#include "thip_encode_mask.h"

namespace thip {

struct SkipOut {          // device memory the launches write beside InterBufs and qii
  uint8_t *skf;           // [nfrags], raster: 1 where the test left the block uncoded
  int64_t *dcode;         // [n], coded order (each may be nullptr): D_code, R, D_skip of every block, coded or not
  int64_t *rate;
  int64_t *dskip;
};

// rows 2j, 2j + 1 of PREV at block (fx, fy) of plane p: the reads clamp like every read of a reference
struct SkipRefBlock {
  const uint8_t *base;   // the plane's column fx * 8
  int stride, h1, y0, w1x;   // w1x: the last column of the plane less fx * 8
  bool dwords;           // two aligned dword reads a row, all eight columns inside
};
__device__ __forceinline__ SkipRefBlock skip_ref_block(const EncRef &R, int p, int fx, int fy) {
  SkipRefBlock s;
  s.base = R.plane[p] + fx * 8;
  s.stride = R.stride[p];
  s.h1 = R.h[p] - 1;
  s.y0 = fy * 8;
  s.w1x = R.w[p] - 1 - fx * 8;
  s.dwords = ((reinterpret_cast<uintptr_t>(R.plane[p]) | (uintptr_t)(uint32_t)s.stride) & 3u) == 0 && s.w1x >= 7;
  return s;
}

// row r of a block's residual (enc_residual_row) and, added to ssd, the row's squared differences of the source against PREV at the
// block's own position.  It keeps its own form of enc_residual_row's two branches: forming enc_residual_row over a shared function of
// the row's pixels moved the resource lines of k_enc_inter_fq (8 bytes of scratch), k_enc_inter_fq_all, k_rate_fdct_inter and
// k_enc_mb_rd
__device__ __forceinline__ void skip_residual_row(int v[8], uint32_t &ssd, const EncSrcBlock &s, const EncPredBlock &b,
                                                  const SkipRefBlock &c, int r) {
  const uint8_t *row = enc_src_row(s, r);
  int px[8];
#pragma unroll
  for (int i = 0; i < 8; i++) px[i] = (int)row[s.cx[i]];
  if (b.intra) {
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = px[i] - 128;
  } else {
    const uint8_t *ra = b.pl + (int64_t)min(max(b.ya + r, 0), b.h1) * b.stride;
    const uint8_t *rb = b.pl + (int64_t)min(max(b.yb + r, 0), b.h1) * b.stride;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = px[i] - (((int)ra[b.ca[i]] + (int)rb[b.cb[i]]) >> 1);
  }
  const uint8_t *rc = c.base + (int64_t)min(c.y0 + r, c.h1) * c.stride;
  if (c.dwords) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(rc);
    const uint32_t wx = w[0], wy = w[1];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int d = px[i] - (int)(((i < 4 ? wx : wy) >> (8 * (i & 3))) & 0xFFu);
      ssd += (uint32_t)(d * d);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int d = px[i] - (int)rc[min(i, c.w1x)];
      ssd += (uint32_t)(d * d);
    }
  }
}

// The body of the four kernels: blocks k0 .. k1 - 1 of the coded order, sixteen a wave from k0 on.  kClasses 2 with k_enc_me's words,
// 3 with k_enc_me_all's.  levels, dcq, qii, cmap, dclast, overflow, dequant ([64 qi][6][64]), bqbits, sel, iscale: enc_fq_bqi's.
// lam_fix: not negative, it stands in for the unscaled lambda of every block.
// cmap is also READ by a chroma block (its macro block's luma entries): the luma range is launched first.
template <int kClasses, bool kMask, class Word>
__device__ __forceinline__ void enc_fq_skip(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap, uint32_t *dclast,
                                            uint32_t *overflow, const SkipOut &so, const int32_t *coded_order, const EncPlanes &g,
                                            const EncRef &R, const EncRef &G, const Word *mbw, int nmbx, const uint16_t *dequant,
                                            const uint8_t *bqbits, const BqiSel &sel, const uint16_t *iscale, int64_t lam_fix, int64_t k0, int64_t k1) {
  constexpr int kTabs = 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;   // (the token kernel counts into it)
  __shared__ __attribute__((aligned(16))) uint2 s_t[3 * kTabs * 64];   // per (qi k, table), by natural position
  __shared__ uint8_t s_bits[2 * 128];                                   // luma, chroma: [4][32]
  for (int i = (int)threadIdx.x; i < sel.nqis * kTabs * 64; i += 256) {
    const int kq = i / (kTabs * 64), t = (i >> 6) % kTabs, z = i & 63;
    const int qi = kq == 0 ? sel.q0 : kq == 1 ? sel.q1 : sel.q2;
    s_t[(kq * kTabs + t) * 64 + kFZigZag[z]] = enc_quant_entry(dequant[(qi * kTabs + t) * 64 + z], z);
  }
  {
    const int i = (int)threadIdx.x;   // (256 threads, 256 bytes)
    s_bits[i] = bqbits[(i < 128 ? sel.tl : sel.tc) * 128 + (i & 127)];
  }
  __shared__ int4 s_x[3][4 * 128];   // per qi of the list and wave; qi 0's is the staging area first
  constexpr int kLv = 4 * 128;
  int4 *lds = s_x[0] + ((int)threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t b0 = k0 + (((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2);
  const int64_t k = b0 + b;
  const bool live = k < k1;
  const int fi = coded_order[min(k, k1 - 1)];   // (a lane past the last block: any block's, it stores nothing)
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  EncPred pr = enc_block_pred(mbw, nmbx, R, G, p, fx, fy);
  const bool four_luma = pr.pix == kEncPixFour && p == 0;
  if (p != 0) {
    // the macro block's four luma blocks: none coded, and the decoder takes it for INTER_NOMV
    const int mb = enc_mb_of(p, fx, fy, R.hdec, R.vdec, nmbx), mby = mb / nmbx, mbx = mb - mby * nmbx;
    const uint8_t *c0 = cmap + (int64_t)(2 * mby) * g.nh[0] + 2 * mbx, *c1 = c0 + g.nh[0];
    if (!(c0[0] | c0[1] | c1[0] | c1[1])) pr = EncPred{kEncPixNomv, 0, 0, R.plane[p]};
  }
  const int tab = (pr.pix == kEncPixIntra ? 0 : 3) + p;
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  const EncPredBlock pb = enc_pred_block(R, pr, p, fx, fy);
  const SkipRefBlock cb = skip_ref_block(R, p, fx, fy);
  uint32_t ssd4 = 0;
  enc_stage_rows(lds, b, j, live, [&](int r, int v[8]) { skip_residual_row(v, ssd4, sb, pb, cb, r); });
  __syncthreads();   // (the tables too)
  int o[16];
  fdct4_lds(lds, b, j, o);
  // the levels at each qi of the list, the block's squared error at z >= 1, and the DC's at qis[0]
  int64_t dist0 = 0, dist1 = 0, dist2 = 0, dcerr = 0;
#pragma unroll 1
  for (int kq = 0; kq < sel.nqis; kq++) {
    int64_t dist = 0, dc = 0;
    quantize4_lds(lds + kq * kLv, s_t + (kq * kTabs + tab) * 64, b, j, o, [&](int z, int c, int lv, int d) {
      const int64_t err = (int64_t)c - (int64_t)lv * d;
      dist += z ? err * err : 0;
      dc += z ? 0 : err * err;
    });
    if (kq == 0) {
      dist0 = dist;
      dcerr = dc;
    } else if (kq == 1) {
      dist1 = dist;
    } else {
      dist2 = dist;
    }
  }
  wave_lds_handover();   // every level of the wave is in LDS
  int rbits = 0;
  if (j < sel.nqis) rbits = bqi_ac_bits(lds + j * kLv, b, s_bits + (p > 0 ? 128 : 0));
  const int lb = lane & ~3;
  const int r0 = __shfl(rbits, lb), r1 = __shfl(rbits, lb + 1), r2 = __shfl(rbits, lb + 2);
  const int64_t d0 = bqi_sum4(dist0), d1 = bqi_sum4(dist1), d2 = bqi_sum4(dist2);
  const int64_t s1 = (int64_t)(s_t[tab * 64 + 1].x & 0xFFFFu);   // qis[0]'s step at zig-zag index 1 (natural position 1)
  int64_t lam = lam_fix >= 0 ? lam_fix : (s1 * s1 * 40) >> 7;   // (lam_fix: thip_enc_skip_stage's, for every block's table)
  if constexpr (kMask) lam = (lam * (int64_t)iscale[fi] + 1024) >> 11;
  const int kb = bqi_choose(sel.nqis, lam, d0, d1, d2, r0, r1, r2);
  const int64_t dk = kb == 0 ? d0 : kb == 1 ? d1 : d2;
  const int rk = kb == 0 ? r0 : kb == 1 ? r1 : r2;
  int4 *chosen = lds + kb * kLv;
  // the DC stays at qis[0]
  if (kb && j == 0) reinterpret_cast<int16_t *>(chosen)[lds_block_at(b, 0)] = reinterpret_cast<const int16_t *>(lds)[lds_block_at(b, 0)];
  wave_lds_handover();
  wave_blocks_out_of(levels, [=](int bb) {
    return lds + __shfl(kb, bb * 4) * kLv;   // (the choice of block bb of the wave)
  }, b0, k1);
  // any level of the block not zero (enc_fq_tail's look at the lane's rows), and the two sides of the test
  const int4 w0 = chosen[lds_block_piece(b, 2 * j)], w1 = chosen[lds_block_piece(b, 2 * j + 1)];
  int nz = (w0.x | w0.y | w0.z | w0.w | w1.x | w1.y | w1.z | w1.w) != 0;
  nz |= __shfl_xor(nz, 1);
  nz |= __shfl_xor(nz, 2);
  const int64_t dcode = dk + bqi_sum4(dcerr);
  const int64_t ssd = bqi_sum4((int64_t)ssd4);
  const int64_t dskip = (16 * ssd) << ((pr.mvx | pr.mvy) != 0 ? 1 : 0);
  if (j != 0 || !live) return;
  dcq[fi] = (int16_t)lds[lds_block_piece(b, 0)].x;
  const int cls = pr.pix == kEncPixIntra ? 1 : kClasses == 3 && enc_pix_gold(pr.pix) ? 3 : 2;
  const bool wanted = pr.pix != kEncPixNomv || nz;
  const bool skipped = wanted && !four_luma && dskip <= dcode + lam * rk;
  const bool coded = wanted && !skipped;
  cmap[fi] = coded ? (uint8_t)cls : (uint8_t)0;
  if (coded) atomicMax(&dclast[(fi >> 8) * kClasses + cls - 1], (uint32_t)fi + 1u);
  qii[k] = (uint8_t)kb;
  so.skf[fi] = skipped ? 1 : 0;
  if (so.dcode) so.dcode[k] = dcode;
  if (so.rate) so.rate[k] = rk;
  if (so.dskip) so.dskip[k] = dskip;
}

// (162 VGPRs, three waves a SIMD where enc_fq_bqi's kernels run four: asked for four (amdgpu_waves_per_eu(4)) the compiler spills 68
// bytes a lane to scratch, and 72 with the SSD gathered in a pass of its own before the staging, so the kernels stay as they are)
#define THIP_SKIP_KERNEL(name, Word, ...)                                                                                            \
  __global__ __launch_bounds__(256) void name(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap, uint32_t *dclast,         \
                                              uint32_t *overflow, SkipOut so, const int32_t *coded_order, EncPlanes g, EncRef R,    \
                                              __VA_ARGS__ const Word *mbw, int nmbx, const uint16_t *dequant, const uint8_t *bqbits, \
                                              BqiSel sel, const uint16_t *iscale, int64_t lam_fix, int64_t k0, int64_t k1)

// k_enc_me's words (five modes): without and with masking's scale
THIP_SKIP_KERNEL(k_enc_inter_fq_skip, uint32_t, ) {
  enc_fq_skip<2, false>(levels, dcq, qii, cmap, dclast, overflow, so, coded_order, g, R, R, mbw, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
}
THIP_SKIP_KERNEL(k_enc_inter_fq_skip_mask, uint32_t, ) {
  enc_fq_skip<2, true>(levels, dcq, qii, cmap, dclast, overflow, so, coded_order, g, R, R, mbw, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
}
// k_enc_me_all's words (eight modes)
THIP_SKIP_KERNEL(k_enc_inter_fq_all_skip, uint4, EncRef G, ) {
  enc_fq_skip<3, false>(levels, dcq, qii, cmap, dclast, overflow, so, coded_order, g, R, G, mbw, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
}
THIP_SKIP_KERNEL(k_enc_inter_fq_all_skip_mask, uint4, EncRef G, ) {
  enc_fq_skip<3, true>(levels, dcq, qii, cmap, dclast, overflow, so, coded_order, g, R, G, mbw, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
}
#undef THIP_SKIP_KERNEL

// ---- the launches, stated once: th_encode_* (thip_encode.hip) and thip_enc_skip_stage (theora_hip.h) both call this ---------------
// The luma blocks of the coded order (its first nluma entries), then the chroma blocks.  Word: k_enc_me's (G is not read) or
// k_enc_me_all's.  iscale: masking's scales, or nullptr without them.  dequant: [64 qi][6][64], of which sel names the frame's list.
// lam_fix: -1 (th_encode_*: every block's lambda from its own table), else the unscaled lambda of every block.
template <class Word>
inline hipError_t skip_launch(const InterBufs &o, uint8_t *qii, const SkipOut &so, const int32_t *order, const EncPlanes &g,
                              const EncRef &R, const EncRef &G, const Word *mb, int nmbx, const uint16_t *dequant,
                              const uint8_t *bqbits, const BqiSel &sel, const uint16_t *iscale, int64_t lam_fix, int64_t n, hipStream_t stream) {
  const int64_t nluma = (int64_t)g.nh[0] * g.nv[0];
  for (int part = 0; part < 2; part++) {
    const int64_t k0 = part ? nluma : 0, k1 = part ? n : nluma;
    if (k1 <= k0) continue;
    const dim3 grid((unsigned)((4 * (k1 - k0) + 255) / 256)), wg(256);
    if constexpr (sizeof(Word) == sizeof(uint4)) {
      if (iscale)
        hipLaunchKernelGGL(k_enc_inter_fq_all_skip_mask, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, so, order,
                           g, R, G, mb, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
      else
        hipLaunchKernelGGL(k_enc_inter_fq_all_skip, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, so, order, g, R,
                           G, mb, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
    } else {
      if (iscale)
        hipLaunchKernelGGL(k_enc_inter_fq_skip_mask, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, so, order, g,
                           R, mb, nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
      else
        hipLaunchKernelGGL(k_enc_inter_fq_skip, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, so, order, g, R, mb,
                           nmbx, dequant, bqbits, sel, iscale, lam_fix, k0, k1);
    }
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

}  // namespace thip
