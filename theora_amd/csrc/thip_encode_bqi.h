// thip_encode_bqi.h -- block-level qi (TH_ENCCTL_THIP_SET_BLOCK_QI; the rule is stated in theoraenc_hip.h, "Block-level qi"): the
// block-qi forms of the three quantising kernels, one body (enc_fq_bqi) over the pieces of the plain ones: enc_quant_entry,
// enc_block_pred, enc_stage_rows with enc_residual_row, enc_fq_tail.  It stages the block's residual, transforms it once (fdct4_lds
// of thip_fdct.h), quantises the coefficients at every qi of the frame's list into LDS (quantize4_lds, whose hook sums the squared
// error), and chooses per block:
//   D_k  each of the block's four lanes sums the squared error of its 16 coefficients (z >= 1) at qi k; two shuffles add them;
//   R_k  lane k of the block walks the AC levels at qi k with enc_value_tokens (enc_block_tokens's classification) and adds the
//        token bits of the previous packet's AC tables (a 256-byte table in LDS);
// then the least D_k + lambda R_k (+ lambda for k != 0).  The chosen levels, with the DC at qis[0], go out as the plain kernel writes
// its levels, with one qii byte a block (coded order).  Four lanes a block, sixteen blocks a wave, as the plain kernels.  The DC,
// token, scan and scatter kernels serve the result unchanged.
#pragma once
#include "thip_encode_modes.h"
#include "thip_rate.h"

namespace thip {

struct BqiSel {      // the frame's qi list and the AC table indices (luma, chroma) of the previous packet of its type
  int nqis, q0, q1, q2, tl, tc;
};

// the bits of block b's AC tokens in lv (zig-zag levels, fdct_quantize4_lds's layout): the walk starts at index 1, the block's own
// EOB included; bits [4][32]: code length + extra bits by (Huffman group - 1, token)
__device__ __forceinline__ int bqi_ac_bits(const int4 *lv, int b, const uint8_t *bits) {
  const int16_t *l16 = reinterpret_cast<const int16_t *>(lv);
  auto level = [&](int z) { return (int)l16[lds_block_at(b, z)]; };
  uint64_t nzm = 0;
#pragma unroll
  for (int pc = 0; pc < 8; pc++) {
    const int4 w = lv[lds_block_piece(b, pc)];
    const int w4[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      nzm |= (uint64_t)((w4[q] & 0xFFFF) != 0) << (pc * 8 + 2 * q);
      nzm |= (uint64_t)((w4[q] >> 16) != 0) << (pc * 8 + 2 * q + 1);
    }
  }
  nzm &= ~1ull;
  int r = 0, next = 1;
  auto count = [&](int t, int, int zs) { r += bits[(zs <= 5 ? 0 : zs <= 14 ? 1 : zs <= 27 ? 2 : 3) * 32 + t]; };
  while (nzm) {
    const int z = __builtin_ctzll(nzm);
    nzm &= nzm - 1;
    enc_value_tokens(level(z), z, next, count);
    next = z + 1;
  }
  if (next < 64) count(0, 0, next);
  return r;
}

__device__ __forceinline__ int64_t bqi_sum4(int64_t v) {   // over the four lanes of a block
#pragma unroll
  for (int m = 1; m <= 2; m <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
    v += (int64_t)((uint64_t)hi << 32 | lo);
  }
  return v;
}

// The choice among the nqis candidates of a block (theoraenc_hip.h, "Block-level qi"): the least D_k + lam R_k, plus lam for k != 0;
// on a tie the lower k.  enc_fq_bqi and enc_fq_skip (thip_encode_skip.h) both choose with it
__device__ __forceinline__ int bqi_choose(int nqis, int64_t lam, int64_t d0, int64_t d1, int64_t d2, int r0, int r1, int r2) {
  int64_t best = d0 + lam * r0;
  int kb = 0;
  if (nqis > 1 && d1 + lam * (r1 + 1) < best) {
    best = d1 + lam * (r1 + 1);
    kb = 1;
  }
  if (nqis > 2 && d2 + lam * (r2 + 1) < best) kb = 2;
  return kb;
}

// The body of the three kernels.  kClasses: the reference classes of enc_fq_tail -- 0 a key frame (no prediction, mbw not read), 2
// with k_enc_me's words, 3 with k_enc_me_all's.  levels [n][64], dcq [nfrags], qii [n] (coded order); inter: cmap, dclast as the
// plain kernels.  dequant: [64 qi][kTabs][64] zig-zag (key: the three intra tables; inter: intra then inter).  bqbits
// [16 tables][4][32]: code length of table t in Huffman group 1..4 + extra bits.  kMask: activity masking (thip_encode_mask.h has
// the kernels): the block's lambda is scaled by iscale[fi] (Q11); else iscale is not read.
template <int kClasses, bool kMask, class Word>
__device__ __forceinline__ void enc_fq_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap, uint32_t *dclast,
                                           uint32_t *overflow, const int32_t *coded_order, const EncPlanes &g, const EncRef &R,
                                           const EncRef &G, const Word *mbw, int nmbx, const uint16_t *dequant, const uint8_t *bqbits,
                                           const BqiSel &sel, int64_t n, const uint16_t *iscale = nullptr) {
  constexpr int kTabs = kClasses ? 6 : 3;
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
  constexpr int kLv = 4 * 128;      // from the wave's levels at one qi to those at the next
  int4 *lds = s_x[0] + ((int)threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t b0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2;
  const int64_t k = b0 + b;
  const int fi = coded_order[min(k, n - 1)];   // (a lane past the last block: any block's, it stores nothing)
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  EncPred pr = {kEncPixIntra, 0, 0, nullptr};
  if constexpr (kClasses != 0) pr = enc_block_pred(mbw, nmbx, R, G, p, fx, fy);
  const int tab = (pr.pix == kEncPixIntra ? 0 : 3) + p;
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  const EncPredBlock pb = enc_pred_block(R, pr, p, fx, fy);
  enc_stage_rows(lds, b, j, k < n, [&](int r, int v[8]) { enc_residual_row(v, sb, pb, r); });
  __syncthreads();   // (the tables too)
  int o[16];
  fdct4_lds(lds, b, j, o);
  // the levels at each qi of the list and the block's squared error at z >= 1
  int64_t dist0 = 0, dist1 = 0, dist2 = 0;
#pragma unroll 1
  for (int kq = 0; kq < sel.nqis; kq++) {
    int64_t dist = 0;
    quantize4_lds(lds + kq * kLv, s_t + (kq * kTabs + tab) * 64, b, j, o, [&](int z, int c, int lv, int d) {
      const int64_t err = (int64_t)c - (int64_t)lv * d;
      dist += z ? err * err : 0;
    });
    if (kq == 0) dist0 = dist;
    else if (kq == 1) dist1 = dist;
    else dist2 = dist;
  }
  wave_lds_handover();   // every level of the wave is in LDS
  int rbits = 0;
  if (j < sel.nqis) rbits = bqi_ac_bits(lds + j * kLv, b, s_bits + (p > 0 ? 128 : 0));
  const int lb = lane & ~3;
  const int r0 = __shfl(rbits, lb), r1 = __shfl(rbits, lb + 1), r2 = __shfl(rbits, lb + 2);
  const int64_t d0 = bqi_sum4(dist0), d1 = bqi_sum4(dist1), d2 = bqi_sum4(dist2);
  const int64_t s1 = (int64_t)(s_t[tab * 64 + 1].x & 0xFFFFu);   // qis[0]'s step at zig-zag index 1 (natural position 1)
  int64_t lam = (s1 * s1 * 40) >> 7;
  if constexpr (kMask) lam = (lam * (int64_t)iscale[fi] + 1024) >> 11;
  const int kb = bqi_choose(sel.nqis, lam, d0, d1, d2, r0, r1, r2);
  int4 *chosen = lds + kb * kLv;
  // the DC stays at qis[0]
  if (kb && j == 0) reinterpret_cast<int16_t *>(chosen)[lds_block_at(b, 0)] = reinterpret_cast<const int16_t *>(lds)[lds_block_at(b, 0)];
  wave_lds_handover();
  enc_fq_tail<kClasses>(levels, dcq, cmap, dclast, lds, [=](int bb) {
    return lds + __shfl(kb, bb * 4) * kLv;   // (the choice of block bb of the wave)
  }, chosen, b0, n, fi, pr.pix);
  if (j == 0 && k < n) qii[k] = (uint8_t)kb;
}

// k_enc_intra_fq with block qi.  dequant: [64 qi][3][64] (the intra tables)
__global__ __launch_bounds__(256) void k_enc_intra_fq_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint32_t *overflow,
                                                          const int32_t *coded_order, EncPlanes g, const uint16_t *dequant,
                                                          const uint8_t *bqbits, BqiSel sel, int64_t n) {
  EncRef R = {};
  enc_fq_bqi<0, false>(levels, dcq, qii, nullptr, nullptr, overflow, coded_order, g, R, R, (const uint32_t *)nullptr, 0, dequant, bqbits,
                sel, n);
}

// k_enc_inter_fq with block qi.  dequant: [64 qi][6][64] (intra, then inter)
__global__ __launch_bounds__(256) void k_enc_inter_fq_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap, uint32_t *dclast,
                                                          uint32_t *overflow, const int32_t *coded_order, EncPlanes g, EncRef R,
                                                          const uint32_t *mb_mode, int nmbx, const uint16_t *dequant,
                                                          const uint8_t *bqbits, BqiSel sel, int64_t n) {
  enc_fq_bqi<2, false>(levels, dcq, qii, cmap, dclast, overflow, coded_order, g, R, R, mb_mode, nmbx, dequant, bqbits, sel, n);
}

// k_enc_inter_fq_all with block qi
__global__ __launch_bounds__(256) void k_enc_inter_fq_all_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap,
                                                              uint32_t *dclast, uint32_t *overflow, const int32_t *coded_order,
                                                              EncPlanes g, EncRef R, EncRef G, const uint4 *mb_word, int nmbx,
                                                              const uint16_t *dequant, const uint8_t *bqbits, BqiSel sel,
                                                              int64_t n) {
  enc_fq_bqi<3, false>(levels, dcq, qii, cmap, dclast, overflow, coded_order, g, R, G, mb_word, nmbx, dequant, bqbits, sel, n);
}

}  // namespace thip
