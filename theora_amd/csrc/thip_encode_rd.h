// thip_encode_rd.h -- the rate-distortion mode decision of an eight-mode inter frame (TH_ENCCTL_THIP_SET_RD_MODES; the rule is stated
// in theoraenc_hip.h, "Rate-distortion mode decision").  Two launches stand in for k_enc_me_all:
//
//   k_enc_me_cand   k_enc_me_all's search without its decision (enc_me_all<true>, thip_encode_modes.h): 32 bytes a macro block, every
//                   candidate's vector and SAD.
//   k_enc_mb_rd     one work group a macro block.  A (candidate, block) pair is a block of the four-lane kernels: sixteen pairs a
//                   wave, sixty-four a pass, the macro block's 36 (4:2:0), 48 (4:2:2) or 72 (4:4:4) pairs in one pass or two.  Each
//                   pair's residual under its candidate is staged (enc_word_pred, enc_pred_block, enc_stage_rows with
//                   enc_residual_row), transformed (fdct4_lds) and quantised at the frame's qi (quantize4_lds, whose hook sums the
//                   squared error and the squared coefficients); bqi_sum4 adds the four lanes' sums; lane 0 of the pair walks the
//                   tokens (enc_value_tokens) and adds their bits from a 2 x 5 x 32-byte table in LDS.  The pairs' D + lambda R go
//                   to LDS, six threads add each candidate's with its header bits, thread 0 takes the least (a tie: the lower
//                   index) and writes k_enc_me_all's word.  No atomics; nothing depends on the order in which waves run.
// Everything behind the words -- the quantising kernels, DC, tokens, the packetiser -- reads them as it reads k_enc_me_all's.
#pragma once
#include "thip_encode_bqi.h"

namespace thip {

// ---- the rule's constants (theoraenc_hip.h states them; tests/enc_rd_ref.py restates them) -------------------------------------
constexpr int kRdLamNum = 40;                                          // lambda = (s1 * s1 * kRdLamNum) >> 7
__device__ constexpr int kRdHeaderBits[6] = {1, 15, 55, 5, 18, 4};     // H_m: a mode code, six bits a component of each vector
__device__ constexpr int kRdPix[6] = {kEncPixNomv, kEncPixMv, kEncPixFour, kEncPixGoldNomv, kEncPixGoldMv, kEncPixIntra};
constexpr int kRdCands = 6;
constexpr int kRdMaxPairs = 72;                                        // 4:4:4: six candidates of twelve blocks

// lambda of the frame whose inter luma step at zig-zag index 1 is s1
inline int64_t rd_lambda(int s1) { return ((int64_t)s1 * s1 * kRdLamNum) >> 7; }

// k_enc_me_all's word of candidate m from the macro block's record (c0: k_enc_me_cand's first uint4): what k_enc_mb_rd predicts
// from and what it writes for the winner
__device__ __forceinline__ uint4 rd_cand_word(const uint4 &c0, int m) {
  const int pix = kRdPix[m];
  const uint32_t v = pix == kEncPixMv ? c0.x & 0xFFFFu : pix == kEncPixGoldMv ? c0.x >> 16 : 0u;
  const bool four = pix == kEncPixFour;
  return make_uint4((uint32_t)pix | v << 8, four ? c0.y : 0u, four ? c0.z : 0u, c0.x >> 16);
}

// the bits of block b's tokens in lv (zig-zag levels, fdct_quantize4_lds's layout) as the rate probe counts a block: the walk
// starts at index 0 with the charged DC `dc` in place of the level there, the block's own EOB included; bits [5][32]: code length +
// extra bits by (Huffman group, token).  allzero: all 64 levels (the real DC among them) are zero
__device__ __forceinline__ int rd_block_bits(const int4 *lv, int b, const uint8_t *bits, int dc, bool &allzero) {
  const int16_t *l16 = reinterpret_cast<const int16_t *>(lv);
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
  allzero = nzm == 0;
  nzm = (nzm & ~1ull) | (uint64_t)(dc != 0);
  int r = 0, next = 0;
  auto count = [&](int t, int, int zs) { r += bits[(zs == 0 ? 0 : zs <= 5 ? 1 : zs <= 14 ? 2 : zs <= 27 ? 3 : 4) * 32 + t]; };
  while (nzm) {
    const int z = __builtin_ctzll(nzm);
    nzm &= nzm - 1;
    enc_value_tokens(z ? (int)l16[lds_block_at(b, z)] : dc, z, next, count);
    next = z + 1;
  }
  if (next < 64) count(0, 0, next);
  return r;
}

// grid: one work group per macro block (raster, rows from the bottom).  cand [nmbs][2]: k_enc_me_cand's records; dequant [2][3][64]
// (zig-zag: the intra then the inter tables of the frame's qi); bits [tables][5][32]: code length + extra bits by table, Huffman
// group and token, of which sel names the four in use (x DC luma, y DC chroma, z AC luma, w AC chroma) -- the 2 x 5 x 32 bytes the
// kernel counts with; lambda: the rule's, 0..2^24.  Out: mb_out [nmbs], k_enc_me_all's words; costs [nmbs][6] (may be null), the six J
__global__ __launch_bounds__(256) void k_enc_mb_rd(uint4 *mb_out, int64_t *costs, const uint4 *cand, EncPlanes g, EncRef R, EncRef G, int nmbx,
                                                   const uint16_t *dequant, const uint8_t *bits, int4 sel, int64_t lambda) {
  __shared__ __attribute__((aligned(16))) uint2 s_t[6 * 64];   // per (intra / inter, plane), by natural position
  __shared__ uint8_t s_bits[2 * 5 * 32];
  __shared__ int4 s_x[4 * 128];
  __shared__ int64_t s_pair[kRdMaxPairs], s_j[kRdCands];
  __shared__ int s_dc0;   // INTRA: luma block 0's quantised DC
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, b = lane >> 2, j = lane & 3;
  const int mb = (int)blockIdx.x, mbx = mb % nmbx, mby = mb / nmbx;
  const int cw = 2 >> R.hdec, ncb = cw * (2 >> R.vdec), nb = 4 + 2 * ncb, npairs = kRdCands * nb;   // chroma fragments a plane, blocks, pairs
  enc_quant_tables(s_t, dequant, 6);
  for (int i = tid; i < 2 * 5 * 32; i += 256) {   // luma then chroma: group 0 from the DC table, 1..4 from the AC table
    const int c = i >= 5 * 32, hg = (i - c * 5 * 32) >> 5;
    const int t = hg ? (c ? sel.w : sel.z) : (c ? sel.y : sel.x);
    s_bits[i] = bits[(t * 5 + hg) * 32 + (i & 31)];
  }
  const uint4 c0 = cand[2 * (int64_t)mb];
  int4 *lds = s_x + w * 128;
#pragma unroll 1
  for (int base = 0; base < npairs; base += 64) {
    const int pi = base + w * 16 + b;
    const bool live = pi < npairs;
    const int m = live ? pi / nb : 0, bi = live ? pi - m * nb : 0;   // (a lane past the last pair: any pair's, it stores nothing)
    int p = 0, fx = 2 * mbx + (bi & 1), fy = 2 * mby + (bi >> 1);
    if (bi >= 4) {
      const int k = bi - 4, kp = k >= ncb ? k - ncb : k;
      p = k >= ncb ? 2 : 1;
      fx = mbx * cw + (kp & (cw - 1));
      fy = (mby << (1 - R.vdec)) + (cw == 2 ? kp >> 1 : kp);
    }
    const EncPred pr = enc_word_pred(rd_cand_word(c0, m), R, G, p, fx, fy);
    const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
    const EncPredBlock pb = enc_pred_block(R, pr, p, fx, fy);
    enc_stage_rows(lds, b, j, live, [&](int r, int v[8]) { enc_residual_row(v, sb, pb, r); });
    __syncthreads();   // (the tables too)
    int o[16];
    fdct4_lds(lds, b, j, o);
    int64_t dist = 0, energy = 0;
    quantize4_lds(lds, s_t + 64 * ((pr.pix == kEncPixIntra ? 0 : 3) + p), b, j, o, [&](int, int c, int lv, int d) {
      const int64_t err = (int64_t)c - (int64_t)lv * d;
      dist += err * err;
      energy += (int64_t)c * c;
    });
    wave_lds_handover();   // every level of the wave is in LDS
    dist = bqi_sum4(dist);
    energy = bqi_sum4(energy);
    const int l0 = (int)reinterpret_cast<const int16_t *>(lds)[lds_block_at(b, 0)];
    if (live && j == 0 && m == 5 && bi == 0) s_dc0 = l0;
    __syncthreads();
    if (live && j == 0) {
      const int dc = m == 5 && bi >= 1 && bi < 4 ? l0 - s_dc0 : l0;
      bool allzero;
      const int r = rd_block_bits(lds, b, s_bits + (p ? 5 * 32 : 0), dc, allzero);
      s_pair[pi] = m == 0 && allzero ? energy : dist + lambda * r;   // an uncoded block of NOMV: no bits, the whole residual
    }
    wave_lds_handover();   // the walk has read the levels; the next pass stages over them
  }
  __syncthreads();
  if (tid < kRdCands) {
    int64_t J = lambda * kRdHeaderBits[tid];
    for (int k = 0; k < nb; k++) J += s_pair[tid * nb + k];
    s_j[tid] = J;
    if (costs) costs[(int64_t)mb * kRdCands + tid] = J;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int m = 1; m < kRdCands; m++)
      if (s_j[m] < s_j[best]) best = m;   // a tie keeps the lower index
    mb_out[mb] = rd_cand_word(c0, best);
  }
}

// ---- the launches, stated once: th_encode_* (thip_encode.hip) and thip_enc_rd_stage (theora_hip.h) both call this ----------------
struct RdBufs {
  uint4 *cand;            // [nmbs][2]: k_enc_me_cand's records
  uint4 *words;           // [nmbs]: k_enc_me_all's words
  int64_t *costs;         // [nmbs][6], or null
};

// search: k_enc_me_cand into o.cand; decide: k_enc_mb_rd over o.cand into o.words (and o.costs).  dequant [2][3][64], bits
// [tables][5][32] with sel: device memory, as k_enc_mb_rd takes them
inline hipError_t rd_launch(const RdBufs &o, bool search, bool decide, const EncPlanes &g, const EncRef &R, const EncRef &G, int nmbx, int nmbs,
                            int lambda_search, int64_t lambda_rd, const uint16_t *dequant, const uint8_t *bits, int4 sel, hipStream_t stream) {
  if (search) {
    hipLaunchKernelGGL(k_enc_me_cand, dim3((unsigned)nmbs), dim3(256), 0, stream, o.cand, g, R, G, nmbx, lambda_search);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  if (decide)
    hipLaunchKernelGGL(k_enc_mb_rd, dim3((unsigned)nmbs), dim3(256), 0, stream, o.words, o.costs, (const uint4 *)o.cand, g, R, G, nmbx, dequant,
                       bits, sel, lambda_rd);
  return hipGetLastError();
}

}  // namespace thip
