// thip_encode_bqi.h -- block-level qi (TH_ENCCTL_THIP_SET_BLOCK_QI; the rule is stated in theoraenc_hip.h, "Block-level qi"): the
// block-qi forms of the three quantising kernels.  Each stages the block's residual as its plain form does (k_enc_intra_fq,
// k_enc_inter_fq, k_enc_inter_fq_all), transforms it once (rate_fdct4_lds: fdct_quantize4_lds's transform), quantises the
// coefficients at every qi of the frame's list into LDS, and chooses per block:
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

enum { kBqiIntra = 0, kBqiInter = 1, kBqiAll = 2 };

struct BqiSel {      // the frame's qi list and the AC table indices (luma, chroma) of the previous packet of its type
  int nqis, q0, q1, q2, tl, tc;
};

// the bits of block b's AC tokens in lv (zig-zag levels, fdct_quantize4_lds's layout): the walk starts at index 1, the block's own
// EOB included; bits [4][32]: code length + extra bits by (Huffman group - 1, token)
__device__ __forceinline__ int bqi_ac_bits(const int4 *lv, int b, const uint8_t *bits) {
  const int16_t *l16 = reinterpret_cast<const int16_t *>(lv);
  auto level = [&](int z) { return (int)l16[(b * 8 + (((z >> 3) + b) & 7)) * 8 + (z & 7)]; };
  uint64_t nzm = 0;
#pragma unroll
  for (int pc = 0; pc < 8; pc++) {
    const int4 w = lv[b * 8 + ((pc + b) & 7)];
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

// The body of the three kernels.  levels [n][64], dcq [nfrags], qii [n] (coded order); inter: cmap, dclast as the plain kernels
// (two classes for kBqiInter, three for kBqiAll).  dequant: [64 qi][kTabs][64] zig-zag (intra: the three intra tables; inter: intra
// then inter).  bqbits [16 tables][4][32]: code length of table t in Huffman group 1..4 + extra bits.
template <int kKind>
__device__ __forceinline__ void enc_fq_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap, uint32_t *dclast,
                                           uint32_t *overflow, const int32_t *coded_order, const EncPlanes &g, const EncRef &R,
                                           const EncRef &G, const void *mbw, int nmbx, const uint16_t *dequant, const uint8_t *bqbits,
                                           const BqiSel &sel, int64_t n) {
  constexpr int kTabs = kKind == kBqiIntra ? 3 : 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;   // (the token kernel counts into it)
  __shared__ __attribute__((aligned(16))) uint2 s_t[3 * kTabs * 64];   // per (qi k, table), by natural position
  __shared__ uint8_t s_bits[2 * 128];                                   // luma, chroma: [4][32]
  for (int i = (int)threadIdx.x; i < sel.nqis * kTabs * 64; i += 256) {
    const int kq = i / (kTabs * 64), t = (i >> 6) % kTabs, z = i & 63, pos = kFZigZag[z];
    const int qi = kq == 0 ? sel.q0 : kq == 1 ? sel.q1 : sel.q2;
    const uint32_t dq = dequant[(qi * kTabs + t) * 64 + z];
    const uint32_t d = dq << 1;   // as k_enc_intra_fq
    const int l = 31 - __builtin_clz(d);
    const uint32_t tt = 1u + ((1u << (16 + l)) / d);
    const int m = (int)(int16_t)(tt - 0x10000u);
    s_t[(kq * kTabs + t) * 64 + pos] = make_uint2(dq | (uint32_t)(uint16_t)m << 16, (uint32_t)(l & 0xFF) | (uint32_t)z << 8);
  }
  {
    const int i = (int)threadIdx.x;   // (256 threads, 256 bytes)
    s_bits[i] = bqbits[(i < 128 ? sel.tl : sel.tc) * 128 + (i & 127)];
  }
  __shared__ int4 s_x[4 * 128], s_l[2][4 * 128];   // per wave: qi 0 (the staging area first), qi 1, qi 2
  const int w = (int)threadIdx.x >> 6;
  int4 *lds = s_x + w * 128, *lv1 = s_l[0] + w * 128, *lv2 = s_l[1] + w * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t b0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2;
  const int64_t k = b0 + b;
  int p = 0, fi = 0, tab = 0, pix = kEncPixIntra;
  if (k < n) {
    fi = coded_order[k];
    p = enc_plane_of(g, fi);
    const int loc = fi - g.froff[p], fy = loc / g.nh[p], fx = loc - fy * g.nh[p];
    int mvx = 0, mvy = 0;
    const uint8_t *pl = nullptr;
    if constexpr (kKind == kBqiInter) {   // k_enc_inter_fq's prediction
      const int mbx = p ? fx >> (1 - R.hdec) : fx >> 1, mby = p ? fy >> (1 - R.vdec) : fy >> 1;
      const uint32_t mw = reinterpret_cast<const uint32_t *>(mbw)[mby * nmbx + mbx];
      pix = (int)(mw & 0xFF);
      mvx = (int)(int8_t)(mw >> 8);
      mvy = (int)(int8_t)(mw >> 16);
      pl = R.plane[p];
    } else if constexpr (kKind == kBqiAll) {   // k_enc_inter_fq_all's
      const int mbx = p ? fx >> (1 - R.hdec) : fx >> 1, mby = p ? fy >> (1 - R.vdec) : fy >> 1;
      const uint4 mw = reinterpret_cast<const uint4 *>(mbw)[mby * nmbx + mbx];
      pix = (int)(mw.x & 0xFF);
      mvx = (int)(int8_t)(mw.x >> 8);
      mvy = (int)(int8_t)(mw.x >> 16);
      if (pix == kEncPixFour) {
        const int row = fy & 1;
        const uint32_t rw = row ? mw.z : mw.y;
        const int ax = (int)(int8_t)rw, ay = (int)(int8_t)(rw >> 8), bx = (int)(int8_t)(rw >> 16), by = (int)(int8_t)(rw >> 24);
        if (p == 0 || (!R.hdec && !R.vdec)) {
          mvx = fx & 1 ? bx : ax;
          mvy = fx & 1 ? by : ay;
        } else if (R.hdec && R.vdec) {
          const uint32_t o = row ? mw.y : mw.z;
          mvx = enc_round_div(ax + bx + (int)(int8_t)o + (int)(int8_t)(o >> 16), 2);
          mvy = enc_round_div(ay + by + (int)(int8_t)(o >> 8) + (int)(int8_t)(o >> 24), 2);
        } else {
          mvx = enc_round_div(ax + bx, 1);
          mvy = enc_round_div(ay + by, 1);
        }
      }
      const uint8_t *pr = R.plane[p], *pg = G.plane[p];   // (both loaded, then the value chosen: choosing the struct copied both to scratch)
      pl = pix == kEncPixGoldNomv || pix == kEncPixGoldMv ? pg : pr;
    }
    tab = (pix == kEncPixIntra ? 0 : 3) + p;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = 2 * j + h, y = fy * 8 + r;
      int v[8];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const int x = fx * 8 + c;
        v[c] = enc_src_px(g, p, x, y) - (pix == kEncPixIntra ? 128 : enc_pred_px_pl(R, pl, p, x, y, mvx, mvy));
      }
      lds[b * 8 + ((r + b) & 7)] = make_int4((v[0] & 0xFFFF) | (v[1] << 16), (v[2] & 0xFFFF) | (v[3] << 16),
                                             (v[4] & 0xFFFF) | (v[5] << 16), (v[6] & 0xFFFF) | (v[7] << 16));
    }
  } else {
    lds[b * 8 + ((2 * j + b) & 7)] = make_int4(0, 0, 0, 0);
    lds[b * 8 + ((2 * j + 1 + b) & 7)] = make_int4(0, 0, 0, 0);
  }
  __syncthreads();   // (the tables too)
  int o[16];
  rate_fdct4_lds(lds, b, j, o);
  // the levels at each qi of the list (fdct_quantize4_lds's quantiser) and the block's squared error at z >= 1
  auto at = [&](int z) { return (b * 8 + (((z >> 3) + b) & 7)) * 8 + (z & 7); };
  int64_t dist0 = 0, dist1 = 0, dist2 = 0;
#pragma unroll 1
  for (int kq = 0; kq < sel.nqis; kq++) {
    int16_t *d16 = reinterpret_cast<int16_t *>(kq == 0 ? lds : kq == 1 ? lv1 : lv2);
    const uint2 *st = s_t + (kq * kTabs + tab) * 64;
    int64_t dist = 0;
#pragma unroll
    for (int q = 0; q < 16; q += 2) {
      const uint4 e = *reinterpret_cast<const uint4 *>(&st[(2 * j + (q >> 3)) * 8 + (q & 7)]);
#pragma unroll
      for (int h2 = 0; h2 < 2; h2++) {
        const uint32_t ex = h2 ? e.z : e.x, ey = h2 ? e.w : e.y;
        const int z = (int)(ey >> 8), d = (int)(ex & 0xFFFFu), m = (int)ex >> 16, l = (int)(ey & 0xFFu);
        const int c = o[q + h2];
        int val = c << 1, lv = 0;
        if (abs(val) >= d) {
          const int sg = val >> 31;
          val += (d + sg) ^ sg;
          lv = sx16(((((m * val) >> 16) + val) >> l) - sg);
        }
        d16[at(z)] = (int16_t)lv;
        const int64_t err = (int64_t)c - (int64_t)lv * d;
        dist += z ? err * err : 0;
      }
    }
    if (kq == 0) dist0 = dist;
    else if (kq == 1) dist1 = dist;
    else dist2 = dist;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every level of the wave is in LDS
  int rbits = 0;
  if (j < sel.nqis) rbits = bqi_ac_bits(j == 0 ? lds : j == 1 ? lv1 : lv2, b, s_bits + (p > 0 ? 128 : 0));
  const int lb = lane & ~3;
  const int r0 = __shfl(rbits, lb), r1 = __shfl(rbits, lb + 1), r2 = __shfl(rbits, lb + 2);
  const int64_t d0 = bqi_sum4(dist0), d1 = bqi_sum4(dist1), d2 = bqi_sum4(dist2);
  const int64_t s1 = (int64_t)(s_t[tab * 64 + 1].x & 0xFFFFu);   // qis[0]'s step at zig-zag index 1 (natural position 1)
  const int64_t lam = (s1 * s1 * 40) >> 7;
  int64_t best = d0 + lam * r0;
  int kb = 0;
  if (sel.nqis > 1 && d1 + lam * (r1 + 1) < best) {
    best = d1 + lam * (r1 + 1);
    kb = 1;
  }
  if (sel.nqis > 2 && d2 + lam * (r2 + 1) < best) kb = 2;
  int4 *chosen = kb == 0 ? lds : kb == 1 ? lv1 : lv2;
  // the DC stays at qis[0]
  if (kb && j == 0) reinterpret_cast<int16_t *>(chosen)[at(0)] = reinterpret_cast<const int16_t *>(lds)[at(0)];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int4 *out = reinterpret_cast<int4 *>(levels) + b0 * 8;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int idx = q * 64 + lane, bb = idx >> 3, pc = idx & 7;
    const int kbb = __shfl(kb, bb * 4);
    const int4 *src = kbb == 0 ? lds : kbb == 1 ? lv1 : lv2;
    const int4 v = src[bb * 8 + ((pc + bb) & 7)];
    if (b0 + bb < n) out[idx] = v;
  }
  const int4 w0 = chosen[b * 8 + ((2 * j + b) & 7)], w1 = chosen[b * 8 + ((2 * j + 1 + b) & 7)];
  int nz = (w0.x | w0.y | w0.z | w0.w | w1.x | w1.y | w1.z | w1.w) != 0;
  nz |= __shfl_xor(nz, 1);
  nz |= __shfl_xor(nz, 2);
  if (j == 0 && k < n) {
    dcq[fi] = (int16_t)lds[b * 8 + (b & 7)].x;
    qii[k] = (uint8_t)kb;
    if constexpr (kKind != kBqiIntra) {
      const int cls = pix == kEncPixIntra ? 1 : (pix == kEncPixGoldNomv || pix == kEncPixGoldMv) ? 3 : 2;
      const bool coded = pix != kEncPixNomv || nz;
      cmap[fi] = coded ? (uint8_t)cls : (uint8_t)0;
      if (coded) atomicMax(&dclast[(fi >> 8) * (kKind == kBqiAll ? 3 : 2) + cls - 1], (uint32_t)fi + 1u);
    }
  }
}

// k_enc_intra_fq with block qi.  dequant: [64 qi][3][64] (the intra tables)
__global__ __launch_bounds__(256) void k_enc_intra_fq_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint32_t *overflow,
                                                          const int32_t *coded_order, EncPlanes g, const uint16_t *dequant,
                                                          const uint8_t *bqbits, BqiSel sel, int64_t n) {
  EncRef R = {};
  enc_fq_bqi<kBqiIntra>(levels, dcq, qii, nullptr, nullptr, overflow, coded_order, g, R, R, nullptr, 0, dequant, bqbits, sel, n);
}

// k_enc_inter_fq with block qi.  dequant: [64 qi][6][64] (intra, then inter)
__global__ __launch_bounds__(256) void k_enc_inter_fq_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap, uint32_t *dclast,
                                                          uint32_t *overflow, const int32_t *coded_order, EncPlanes g, EncRef R,
                                                          const uint32_t *mb_mode, int nmbx, const uint16_t *dequant,
                                                          const uint8_t *bqbits, BqiSel sel, int64_t n) {
  enc_fq_bqi<kBqiInter>(levels, dcq, qii, cmap, dclast, overflow, coded_order, g, R, R, mb_mode, nmbx, dequant, bqbits, sel, n);
}

// k_enc_inter_fq_all with block qi
__global__ __launch_bounds__(256) void k_enc_inter_fq_all_bqi(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap,
                                                              uint32_t *dclast, uint32_t *overflow, const int32_t *coded_order,
                                                              EncPlanes g, EncRef R, EncRef G, const uint4 *mb_word, int nmbx,
                                                              const uint16_t *dequant, const uint8_t *bqbits, BqiSel sel,
                                                              int64_t n) {
  enc_fq_bqi<kBqiAll>(levels, dcq, qii, cmap, dclast, overflow, coded_order, g, R, G, mb_word, nmbx, dequant, bqbits, sel, n);
}

}  // namespace thip
