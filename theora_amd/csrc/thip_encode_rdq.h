// thip_encode_rdq.h -- the level choice of th_encode_* (TH_ENCCTL_THIP_SET_RD_QUANT; the rule is stated in theoraenc_hip.h, "Level
// choice"): one kernel body (enc_rdq) behind the frame's quantising kernels, over the pieces they are made of: enc_frag_xy,
// enc_block_pred, enc_src_block / enc_pred_block, enc_stage_rows with enc_residual_row, fdct4_lds, enc_quant_entry for the steps,
// enc_value_tokens and the 256-byte bits table of the block-qi kernels, wave_blocks_in / _out.  It stages the block's residual and
// transforms it as the quantising kernel did (the same code on the same pixels: the same c), READS the block's levels, and per block
//   dd    each of the block's four lanes writes, for its sixteen coefficients with a level that is not zero, what the alternative
//         level adds to the squared error (int64, LDS), and sums the squared error of the levels as they are; two shuffles add those;
//   walk  the block's first lane runs the backward programme (rdq_walk below) over the non-zero positions with F and the choices in
//         LDS, then walks forward through the choices and rewrites the levels in LDS;
// and the wave's levels go back where they came from.  Four lanes a block, sixteen blocks a wave, as the quantising kernels; two
// waves a work group, for each wave holds 19.3 KB of LDS.  No atomics but the frame's sums (integer adds: their order does not matter).
//
// The programme itself (rdq_walk, with the indexing of its arrays) depends on nothing else in this file or outside it: with
// THIP_RDQ_WALK_ONLY defined a host program can include this header alone (tests/native/rdq_walk_host.cpp does, under sanitizers).
#pragma once
#ifndef THIP_RDQ_WALK_ONLY
#include "thip_encode_mask.h"
#endif

namespace thip {

// ---- the programme ---------------------------------------------------------------------------------------------------------------
// A wave's arrays: F and dd are int64 [16 blocks][65], the choices bytes [16][68] -- a block's entries z = 0..63, padded so that the
// sixteen walking lanes of a wave, each at its own z, spread over the LDS banks (strides of 130 and 17 dwords).
constexpr int kRdqStride = 65, kRdqChoiceStride = 68;
__device__ __forceinline__ int rdq_at(int b, int z) { return b * kRdqStride + z; }
__device__ __forceinline__ int rdq_choice_at(int b, int z) { return b * kRdqChoiceStride + z; }

struct RdqCount {
  int zeroed, lowered;   // levels +-1 that became 0, levels |l| >= 2 that became l - sgn(l)
};

// The choice of block b's levels: nzm the zig-zag indices z >= 1 at which its level is not zero; lam = lambda_q (not 0: the caller
// leaves the block alone then); dd[rdq_at(b, z)] what the alternative at z adds to the squared error; level(z) reads a level,
// set(z, v) writes one; vbits(v, z, next) the bits of the tokens that code the value v at z when the block's previous token ended
// before index `next`, ebits(next) those of an EOB at `next`.  F[rdq_at(b, z)] becomes the least cost of everything behind a kept
// level at z (z = 0: the whole block, which is returned: J(a) less the squared error of the levels as they came), choice its
// minimiser: the next kept position, 0 for the EOB, | 0x80 when that position takes its alternative.  Candidates are tried in
// the order "the next non-zero level as it is, its alternative, the one after as it is, ..." and replace the best only when strictly
// less: the first minimiser in lexicographic order of a.
template <class Level, class Set, class VBits, class EBits>
__device__ __forceinline__ int64_t rdq_walk(uint64_t nzm, int64_t lam, int64_t *F, const int64_t *dd, uint8_t *choice, int b,
                                            Level &&level, Set &&set, VBits &&vbits, EBits &&ebits, RdqCount &cnt) {
  uint64_t todo = nzm;   // the states still to do, from the last non-zero position down; then state 0
  for (;;) {
    const int zi = todo ? 63 - __builtin_clzll(todo) : 0;
    uint64_t rest = zi == 63 ? 0ull : nzm & (~0ull << (zi + 1));
    int64_t best = INT64_MAX, acc = 0;   // acc: what the +-1 passed over so far add by becoming 0
    int bc = 0;
    bool open = true;                    // no |l| >= 2 met: the EOB is allowed
    while (rest) {
      const int zj = __builtin_ctzll(rest);
      rest &= rest - 1;
      const int l = level(zj);
      const int64_t behind = acc + F[rdq_at(b, zj)];
      int64_t cost = behind + lam * vbits(l, zj, zi + 1);
      if (cost < best) {
        best = cost;
        bc = zj;
      }
      if (l >= 2 || l <= -2) {
        cost = behind + dd[rdq_at(b, zj)] + lam * vbits(l - (l > 0 ? 1 : -1), zj, zi + 1);
        if (cost < best) {
          best = cost;
          bc = zj | 0x80;
        }
        open = false;
        break;
      }
      acc += dd[rdq_at(b, zj)];
    }
    if (open) {
      const int64_t cost = acc + (zi < 63 ? lam * ebits(zi + 1) : 0);
      if (cost < best) {
        best = cost;
        bc = 0;
      }
    }
    F[rdq_at(b, zi)] = best;
    choice[rdq_choice_at(b, zi)] = (uint8_t)bc;
    if (!todo) break;
    todo &= ~(1ull << zi);
  }
  // forward through the choices
  cnt.zeroed = cnt.lowered = 0;
  for (int z = 0;;) {
    const int c = choice[rdq_choice_at(b, z)], zj = c & 63;
    uint64_t gone = z == 63 ? 0ull : nzm & (~0ull << (z + 1));   // the +-1 between z and the next kept position
    if (zj) gone &= (1ull << zj) - 1;
    while (gone) {
      set(__builtin_ctzll(gone), 0);
      gone &= gone - 1;
      cnt.zeroed++;
    }
    if (!zj) break;
    if (c & 0x80) {
      const int l = level(zj);
      set(zj, l - (l > 0 ? 1 : -1));
      cnt.lowered++;
    }
    z = zj;
  }
  return F[rdq_at(b, 0)];
}

#ifndef THIP_RDQ_WALK_ONLY
// ---- the kernel ------------------------------------------------------------------------------------------------------------------
constexpr int kRdqThreads = 128;   // two waves a work group
enum { kRdqZeroed = 0, kRdqLowered = 3, kRdqEmptied = 6, kRdqRateBefore, kRdqRateAfter, kRdqDistBefore, kRdqDistAfter, kRdqSums };

struct RdqOut {           // device memory beside the levels; each may be nullptr
  int64_t *jbefore;       // [n], coded order: J of the levels as they came, J as they went, R as they went; 0 for an uncoded block
  int64_t *jafter;
  int64_t *rate;
  unsigned long long *sums;   // [kRdqSums]: the frame's, ADDED to (the caller zeroes them)
};

// The body: blocks 0 .. n - 1 of the coded order, sixteen a wave.  kClasses: 0 a key frame (no prediction; mbw, cmap not read), 2 with
// k_enc_me's words, 3 with k_enc_me_all's.  levels [n][64] in and out; qii [n] (coded order) or nullptr (every block at qis[0]); cmap
// [nfrags] raster; dequant [64 qi][ntabs][64] zig-zag, ntabs 3 (the intra tables) or 6 (intra, then inter); bqbits, sel: the block-qi
// kernels'; iscale: masking's scales or nullptr; lam_fix: not negative, it stands in for the unscaled lambda of every block; w the weight.
template <int kClasses, class Word>
__device__ __forceinline__ void enc_rdq(int16_t *levels, const uint8_t *qii, const uint8_t *cmap, const RdqOut &out,
                                        const int32_t *coded_order, const EncPlanes &g, const EncRef &R, const EncRef &G, const Word *mbw,
                                        int nmbx, const uint16_t *dequant, int ntabs, const uint8_t *bqbits, const BqiSel &sel,
                                        const uint16_t *iscale, int64_t lam_fix, int w, int64_t n) {
  constexpr int kWaves = kRdqThreads / 64;
  __shared__ __attribute__((aligned(16))) uint2 s_t[3 * 6 * 64];   // per (qi k, table), by natural position
  __shared__ uint8_t s_bits[2 * 128];                               // luma, chroma: [4][32]
  __shared__ int4 s_x[kWaves * 128];                                // per wave: the staging area, then the levels
  __shared__ int64_t s_dd[kWaves * 16 * kRdqStride], s_f[kWaves * 16 * kRdqStride];
  __shared__ uint8_t s_choice[kWaves * 16 * kRdqChoiceStride];
  __shared__ unsigned long long s_sums[kRdqSums];
  for (int i = (int)threadIdx.x; i < sel.nqis * ntabs * 64; i += kRdqThreads) {
    const int kq = i / (ntabs * 64), t = (i >> 6) % ntabs, z = i & 63;
    const int qi = kq == 0 ? sel.q0 : kq == 1 ? sel.q1 : sel.q2;
    s_t[(kq * ntabs + t) * 64 + kFZigZag[z]] = enc_quant_entry(dequant[(qi * ntabs + t) * 64 + z], z);
  }
  for (int i = (int)threadIdx.x; i < 256; i += kRdqThreads) s_bits[i] = bqbits[(i < 128 ? sel.tl : sel.tc) * 128 + (i & 127)];
  if (threadIdx.x < kRdqSums) s_sums[threadIdx.x] = 0;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  int4 *lds = s_x + wave * 128;
  int64_t *dd = s_dd + wave * 16 * kRdqStride, *F = s_f + wave * 16 * kRdqStride;
  uint8_t *choice = s_choice + wave * 16 * kRdqChoiceStride;
  const int64_t b0 = ((int64_t)blockIdx.x * kRdqThreads + (threadIdx.x & ~63u)) >> 2;
  const int64_t k = b0 + b;
  const bool live = k < n;
  const int fi = coded_order[min(k, n - 1)];   // (a lane past the last block: any block's, it stores nothing)
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  EncPred pr = {kEncPixIntra, 0, 0, nullptr};
  bool coded = live;
  if constexpr (kClasses != 0) {
    pr = enc_block_pred(mbw, nmbx, R, G, p, fx, fy);
    if (p != 0) {
      // the macro block's four luma blocks: none coded, and the decoder takes it for INTER_NOMV ("Skip decision")
      const int mb = enc_mb_of(p, fx, fy, R.hdec, R.vdec, nmbx), mby = mb / nmbx, mbx = mb - mby * nmbx;
      const uint8_t *c0 = cmap + (int64_t)(2 * mby) * g.nh[0] + 2 * mbx, *c1 = c0 + g.nh[0];
      if (!(c0[0] | c0[1] | c1[0] | c1[1])) pr = EncPred{kEncPixNomv, 0, 0, R.plane[p]};
    }
    coded = live && cmap[fi] != 0;
  }
  const int tab = (pr.pix == kEncPixIntra ? 0 : 3) + p;
  const int kq = qii && live ? min((int)qii[k], sel.nqis - 1) : 0;
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  const EncPredBlock pb = enc_pred_block(R, pr, p, fx, fy);
  enc_stage_rows(lds, b, j, live, [&](int r, int v[8]) { enc_residual_row(v, sb, pb, r); });
  __syncthreads();   // (the tables too)
  int o[16];
  fdct4_lds(lds, b, j, o);
  wave_blocks_in(lds, levels, b0, n);
  wave_lds_handover();   // every level of the wave is in LDS
  // what each alternative adds to the squared error, and the squared error of the levels as they are (z >= 1)
  int16_t *l16 = reinterpret_cast<int16_t *>(lds);
  int64_t dist = 0;
  if (live) {
    lane_entries4(s_t + (kq * ntabs + tab) * 64, j, [&](int kk, const QuantEntry &e) {
      const int l = (int)l16[lds_block_at(b, e.z)];
      const int64_t err = (int64_t)o[kk] - (int64_t)l * e.d;
      dist += e.z ? err * err : 0;
      if (l != 0 && e.z != 0) {
        const int64_t alt = (int64_t)o[kk] - (int64_t)(l - (l > 0 ? 1 : -1)) * e.d;
        dd[rdq_at(b, e.z)] = alt * alt - err * err;
      }
    });
  }
  const int64_t d0 = bqi_sum4(dist);
  wave_lds_handover();
  const uint8_t *bits = s_bits + (p > 0 ? 128 : 0);
  if (j == 0 && coded) {
    const int64_t s1 = (int64_t)(s_t[tab * 64 + 1].x & 0xFFFFu);   // qis[0]'s step at zig-zag index 1 (natural position 1)
    int64_t lam = lam_fix >= 0 ? lam_fix : (s1 * s1 * 40) >> 7;
    if (iscale) lam = (lam * (int64_t)iscale[fi] + 1024) >> 11;
    lam = (lam * w) >> 4;
    const int r0 = bqi_ac_bits(lds, b, bits);
    int64_t jb = d0 + lam * r0, ja = jb;
    int r1 = r0;
    RdqCount cnt = {0, 0};
    uint64_t nzm = 0;
#pragma unroll
    for (int pc = 0; pc < 8; pc++) {
      const int4 wv = lds[lds_block_piece(b, pc)];
      const int w4[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        nzm |= (uint64_t)((w4[q] & 0xFFFF) != 0) << (pc * 8 + 2 * q);
        nzm |= (uint64_t)((w4[q] >> 16) != 0) << (pc * 8 + 2 * q + 1);
      }
    }
    nzm &= ~1ull;
    if (lam != 0 && nzm) {
      auto group = [](int zs) { return (zs <= 5 ? 0 : zs <= 14 ? 1 : zs <= 27 ? 2 : 3) * 32; };
      ja = d0 + rdq_walk(nzm, lam, F, dd, choice, b, [&](int z) { return (int)l16[lds_block_at(b, z)]; },
                         [&](int z, int v) { l16[lds_block_at(b, z)] = (int16_t)v; },
                         [&](int v, int z, int next) {
                           int r = 0;
                           enc_value_tokens(v, z, next, [&](int t, int, int zs) { r += bits[group(zs) + t]; });
                           return r;
                         },
                         [&](int next) { return (int)bits[group(next)]; }, cnt);
      r1 = bqi_ac_bits(lds, b, bits);
    }
    if (out.jbefore) out.jbefore[k] = jb;
    if (out.jafter) out.jafter[k] = ja;
    if (out.rate) out.rate[k] = r1;
    if (out.sums) {
      if (cnt.zeroed) atomicAdd(&s_sums[kRdqZeroed + p], (unsigned long long)cnt.zeroed);
      if (cnt.lowered) atomicAdd(&s_sums[kRdqLowered + p], (unsigned long long)cnt.lowered);
      if (cnt.zeroed == __popcll(nzm) && cnt.zeroed) atomicAdd(&s_sums[kRdqEmptied], 1ull);
      atomicAdd(&s_sums[kRdqRateBefore], (unsigned long long)r0);
      atomicAdd(&s_sums[kRdqRateAfter], (unsigned long long)r1);
      atomicAdd(&s_sums[kRdqDistBefore], (unsigned long long)d0);
      atomicAdd(&s_sums[kRdqDistAfter], (unsigned long long)(ja - lam * r1));
    }
  } else if (j == 0 && live) {
    if (out.jbefore) out.jbefore[k] = 0;
    if (out.jafter) out.jafter[k] = 0;
    if (out.rate) out.rate[k] = 0;
  }
  wave_lds_handover();
  wave_blocks_out(levels, lds, b0, n);
  __syncthreads();
  if (out.sums && threadIdx.x < kRdqSums && s_sums[threadIdx.x]) atomicAdd(&out.sums[threadIdx.x], s_sums[threadIdx.x]);
}

#define THIP_RDQ_KERNEL(name, Word, ...)                                                                                               \
  __global__ __launch_bounds__(kRdqThreads) void name(int16_t *levels, const uint8_t *qii, const uint8_t *cmap, RdqOut out,           \
                                                      const int32_t *coded_order, EncPlanes g, EncRef R, __VA_ARGS__ const Word *mbw, \
                                                      int nmbx, const uint16_t *dequant, int ntabs, const uint8_t *bqbits, BqiSel sel, \
                                                      const uint16_t *iscale, int64_t lam_fix, int w, int64_t n)
THIP_RDQ_KERNEL(k_enc_rdq_key, uint32_t, ) {   // a key frame: R is not read
  enc_rdq<0>(levels, qii, cmap, out, coded_order, g, R, R, mbw, nmbx, dequant, ntabs, bqbits, sel, iscale, lam_fix, w, n);
}
THIP_RDQ_KERNEL(k_enc_rdq, uint32_t, ) {       // k_enc_me's words (five modes)
  enc_rdq<2>(levels, qii, cmap, out, coded_order, g, R, R, mbw, nmbx, dequant, ntabs, bqbits, sel, iscale, lam_fix, w, n);
}
THIP_RDQ_KERNEL(k_enc_rdq_all, uint4, EncRef G, ) {   // k_enc_me_all's words (eight modes)
  enc_rdq<3>(levels, qii, cmap, out, coded_order, g, R, G, mbw, nmbx, dequant, ntabs, bqbits, sel, iscale, lam_fix, w, n);
}
#undef THIP_RDQ_KERNEL

// ---- the launch, stated once: th_encode_* (thip_encode.hip) and thip_enc_rdq_stage (theora_hip.h) both call this -----------------
// classes 0 (a key frame: R, G, mb not read), 2 (Word uint32_t) or 3 (Word uint4).  lam_fix: -1 (th_encode_*: every block's lambda
// from its own table), else the unscaled lambda of every block.
template <class Word>
inline hipError_t rdq_launch(int classes, int16_t *levels, const uint8_t *qii, const uint8_t *cmap, const RdqOut &out, const int32_t *order,
                             const EncPlanes &g, const EncRef &R, const EncRef &G, const Word *mb, int nmbx, const uint16_t *dequant,
                             int ntabs, const uint8_t *bqbits, const BqiSel &sel, const uint16_t *iscale, int64_t lam_fix, int w, int64_t n,
                             hipStream_t stream) {
  const dim3 grid((unsigned)((4 * n + kRdqThreads - 1) / kRdqThreads)), wg(kRdqThreads);
  if constexpr (sizeof(Word) == sizeof(uint4)) {
    hipLaunchKernelGGL(k_enc_rdq_all, grid, wg, 0, stream, levels, qii, cmap, out, order, g, R, G, mb, nmbx, dequant, ntabs, bqbits, sel,
                       iscale, lam_fix, w, n);
  } else if (classes == 0) {
    hipLaunchKernelGGL(k_enc_rdq_key, grid, wg, 0, stream, levels, qii, cmap, out, order, g, R, mb, nmbx, dequant, ntabs, bqbits, sel, iscale,
                       lam_fix, w, n);
  } else {
    hipLaunchKernelGGL(k_enc_rdq, grid, wg, 0, stream, levels, qii, cmap, out, order, g, R, mb, nmbx, dequant, ntabs, bqbits, sel, iscale,
                       lam_fix, w, n);
  }
  return hipGetLastError();
}
#endif   // THIP_RDQ_WALK_ONLY

}  // namespace thip
