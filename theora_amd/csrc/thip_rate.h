// thip_rate.h -- the rate probe of th_encode_*'s bitrate mode (thip_encode.hip; the controller and E[q] are stated in
// theoraenc_hip.h, "Bitrate mode").  Before a frame is coded, the probe measures its token bits E[q] at every qi q = 0..63 at once:
// the 64 lanes of a wave are the 64 qi, a wave takes one block.  The quality-mode kernels are not touched; the probe has its own.
//
//   k_rate_me          (inter frames) k_enc_me's search (enc_me_search, thip_encode_inter.h), writing the qi-independent statistics
//                      of each macro block instead of a mode: S0, Smv, SI and the half-pel vector.  The mode at q then follows
//                      from them and q's lambda (rate_mode).
//   k_rate_fdct_key    the unquantised fDCT of every block (raster order, natural order in the block): fdct4_lds of
//                      thip_fdct.h, the transform of every four-lane kernel.
//   k_rate_fdct_inter  the same for the three residuals an inter block may code: INTRA (pixel - 128), NOMV (PREV, vector 0) and MV
//                      (PREV through the macro block's vector) -- [3][nfrags][64].  Both stage their residuals as the frame's
//                      kernels do (enc_stage_rows, enc_residual_row).
//   k_rate_dc          one wave a block, lane q: the block's quantised DC at q, and (inter) whether the block is coded at q and in
//                      which class (ballots into one 64-bit word each).
//   k_rate_tok         a persistent grid, one wave a block, lane q: DC prediction at q, the AC levels at q and the block's tokens,
//                      counted into the work group's LDS histogram [q][luma / chroma][Huffman group][token] (u16 pairs).  The
//                      levels are walked over the indices that are non-zero at ANY q (a ballot against the floor, the least step
//                      over q of each (table, z): rate_form_floor of thip_quant.h.  With steps that fall with q, the built-in
//                      ones, the floor is the step at qi 63), so a sparse block costs a few iterations.  The quantiser tables of the frame type sit in LDS beside the
//                      histogram (48 KB key, 96 KB inter).  Each work group writes its histogram once, as a partial.
//   k_rate_bits        one work group per q (one group alone reads the partials too slowly): the partials summed, the least bits of
//                      each of the four table choices (the setup's code lengths), the extra bits and the frame header -> E[q] (int64;
//                      the host reads back 512 bytes).
#pragma once
#include "thip_encode_inter.h"
#include "thip_quant.h"

namespace thip {

constexpr int kRateBins = 2 * 5 * 32;        // luma / chroma, Huffman group, token
constexpr int kRateHistStride = 161;         // u16-pair words a qi in LDS: 160 + 1, so the 64 lanes spread over the 64 banks
constexpr int kRatePartial = kRateBins + 1;  // a partial's row per qi: the bins and the side count (M, V of the inter estimate)
constexpr int kRateTokWaves = 16;             // waves a work group of k_rate_tok (four a SIMD: the histogram allows one group a CU)
// A u16 bin of k_rate_tok's histogram holds what one lane (one qi) counts over all the blocks its work group takes.  One block adds
// at most 36 to one bin: a bin is one token starting in one Huffman group, the largest group is the indices 28..63, and a token
// starts at an index once.  rate_groups keeps a group's blocks at or below 960 + 16 = 976 (976 * 36 = 35136), and
// thip_enc_rate_stage refuses a caller's count that would give a group kRateBlocksPerGroupLimit blocks or more (1019 * 36 = 36684):
// both stay below 65536.  tests/test_rate_stage_cpu.py derives the 36 from the reference's token counting and checks both products
// (test_grid_rule_keeps_every_bin_below_16_bits); tests/test_gpu_rate_direct.py loads one bin with it (test_tok_heaviest_bin).
constexpr int kRateMaxBlocksPerGroup = 960;
constexpr int kRateBlocksPerGroupLimit = 1020;

// one coefficient through the quantiser, table entry (d | m << 16, l): enc_quant_entry's with zig-zag index 0
__device__ __forceinline__ int rate_quant(int coef, uint2 e) {
  const QuantEntry f = quant_entry_fields(e.x, e.y);
  return quant_level(coef, f.d, f.m, f.l, [] {});
}

// the table entry of rate_quant from its first word: l follows from the step
__device__ __forceinline__ uint2 rate_entry(uint32_t x) {
  int m, l;
  quant_recip((x & 0xFFFFu) << 1, m, l);
  return make_uint2(x, (uint32_t)l);
}

// the four lanes of a block store its 64 coefficients (natural order) at out[0..63]
__device__ __forceinline__ void rate_store16(int16_t *out, int j, const int o[16]) {
  int4 *d = reinterpret_cast<int4 *>(out + 16 * j);
  d[0] = make_int4((o[0] & 0xFFFF) | (o[1] << 16), (o[2] & 0xFFFF) | (o[3] << 16), (o[4] & 0xFFFF) | (o[5] << 16),
                   (o[6] & 0xFFFF) | (o[7] << 16));
  d[1] = make_int4((o[8] & 0xFFFF) | (o[9] << 16), (o[10] & 0xFFFF) | (o[11] << 16), (o[12] & 0xFFFF) | (o[13] << 16),
                   (o[14] & 0xFFFF) | (o[15] << 16));
}

// grid: ceil(4 nfrags / 256).  coef [nfrags][64] int16, natural order, raster fragment order
__global__ __launch_bounds__(256) void k_rate_fdct_key(int16_t *coef, EncPlanes g, int64_t nfrags) {
  __shared__ int4 s_x[4 * 128];
  int4 *lds = s_x + (threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t fi = (((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2) + b;
  int p = 0, fx = 0, fy = 0;
  if (fi < nfrags) enc_frag_xy(g, (int)fi, p, fx, fy);
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  EncPredBlock pb = {};
  pb.intra = true;   // pixel - 128
  enc_stage_rows(lds, b, j, fi < nfrags, [&](int r, int v[8]) { enc_residual_row(v, sb, pb, r); });
  __syncthreads();
  int o[16];
  fdct4_lds(lds, b, j, o);
  if (fi < nfrags) rate_store16(coef + fi * 64, j, o);
}

// the macro block's word of k_rate_me: x = S0, y = Smv, z = SI, w = mvx & 0xFF | (mvy & 0xFF) << 8 (the half-pel vector)
__device__ __forceinline__ int rate_mode(uint4 s, int lambda) {
  int mode = (int)s.y + lambda < (int)s.x ? kEncPixMv : kEncPixNomv;
  const int sinter = mode == kEncPixMv ? (int)s.y : (int)s.x;
  if ((int)s.z + 4 * lambda < sinter) mode = kEncPixIntra;
  return mode;
}

// enc_me_search (thip_encode_inter.h) with the decision left out: S0, Smv, SI and the vector, written as rate_mode's statistics
__global__ __launch_bounds__(256) void k_rate_me(uint4 *mb_out, EncPlanes g, EncRef R, int nmbx) {
  EncMe m;
  if (enc_me_search(m, g, R, nmbx))
    mb_out[blockIdx.x] = make_uint4((uint32_t)m.s0, (uint32_t)m.smv, (uint32_t)m.si, ((uint32_t)m.mvx & 0xFFu) | ((uint32_t)m.mvy & 0xFFu) << 8);
}

// the launch, stated once (the probe, the cut measurement and thip_enc_inter_stage): k_rate_me's word of each of the nmbs macro blocks
inline hipError_t rate_launch_me(uint4 *mb, const EncPlanes &g, const EncRef &R, int nmbx, int nmbs, hipStream_t stream) {
  hipLaunchKernelGGL(k_rate_me, dim3((unsigned)nmbs), dim3(256), 0, stream, mb, g, R, nmbx);
  return hipGetLastError();
}

// grid: ceil(4 nfrags / 256).  coef [3][nfrags][64]: the INTRA, NOMV and MV residuals' coefficients (natural order, raster)
__global__ __launch_bounds__(256) void k_rate_fdct_inter(int16_t *coef, EncPlanes g, EncRef R, const uint4 *mbs, int nmbx,
                                                         int64_t nfrags) {
  __shared__ int4 s_x[4 * 128];
  int4 *lds = s_x + (threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t fi = (((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2) + b;
  int p = 0, fx = 0, fy = 0, mvx = 0, mvy = 0;
  if (fi < nfrags) {
    enc_frag_xy(g, (int)fi, p, fx, fy);
    const uint32_t w = mbs[enc_mb_of(p, fx, fy, R.hdec, R.vdec, nmbx)].w;
    mvx = (int)(int8_t)(w & 0xFF);
    mvy = (int)(int8_t)(w >> 8);
  }
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  for (int v = 0; v < 3; v++) {   // INTRA, NOMV, MV
    const EncPred pr = {v == 0 ? kEncPixIntra : kEncPixMv, v == 2 ? mvx : 0, v == 2 ? mvy : 0, R.plane[p]};
    const EncPredBlock pb = enc_pred_block(R, pr, p, fx, fy);
    enc_stage_rows(lds, b, j, fi < nfrags, [&](int r, int px[8]) { enc_residual_row(px, sb, pb, r); });
    __syncthreads();
    int o[16];
    fdct4_lds(lds, b, j, o);
    if (fi < nfrags) rate_store16(coef + ((int64_t)v * nfrags + fi) * 64, j, o);
    __syncthreads();   // (the next residual reuses the LDS)
  }
}

// What lane q of a wave knows about block fi at q: which residual it codes (0 INTRA, 1 NOMV, 2 MV) and with which table (0..2
// intra of the plane, 3..5 inter); key frames: always (0, plane).
struct RateSel {
  int var, tab, mode;
};
template <bool kInter>
__device__ __forceinline__ RateSel rate_select(const uint4 *mbs, const int *lam, int p, int fx, int fy, int hdec, int vdec, int nmbx,
                                               int q) {
  if (!kInter) return {0, p, kEncPixIntra};
  const int mode = rate_mode(mbs[enc_mb_of(p, fx, fy, hdec, vdec, nmbx)], lam[q]);
  return {mode == kEncPixIntra ? 0 : mode == kEncPixNomv ? 1 : 2, (mode == kEncPixIntra ? 0 : 3) + p, mode};
}

struct RateArgs {
  const int16_t *coef;   // [1 or 3][nfrags][64] natural order
  const uint2 *tab;      // [6 tables][64 z][64 q]: (d | m << 16, l) of oc_enc_quantize
  const uint4 *mbs;      // k_rate_me's words (inter)
  const int *lam;        // [64]: the inter luma step at zig-zag index 1 of each qi
  const uint16_t *floor; // [6 tables][64 z]: the least step over q (rate_form_floor)
  int nmbx, hdec, vdec;
};

// grid: ceil(nfrags / 4), one wave a block.  qdc [nfrags][64]: the quantised DC at each q; (inter) coded, cls [nfrags]: bit q =
// coded at q, of class PREV at q
template <bool kInter>
__global__ __launch_bounds__(256) void k_rate_dc(int16_t *qdc, uint64_t *coded, uint64_t *cls, RateArgs a, EncPlanes g,
                                                 int64_t nfrags) {
  const int q = (int)threadIdx.x & 63;
  const int64_t fi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (fi >= nfrags) return;   // (wave-uniform)
  int p, fx, fy;
  enc_frag_xy(g, (int)fi, p, fx, fy);
  const RateSel s = rate_select<kInter>(a.mbs, a.lam, p, fx, fy, a.hdec, a.vdec, a.nmbx, q);
  const int16_t *cb = a.coef + ((int64_t)s.var * nfrags + fi) * 64;
  qdc[fi * 64 + q] = (int16_t)rate_quant(cb[0], a.tab[(s.tab * 64 + 0) * 64 + q]);
  if (!kInter) return;
  // a NOMV block is coded when a level is not zero: test the indices that are non-zero under the floor (a superset at every q)
  const int16_t *cn = a.coef + (nfrags + fi) * 64;
  const int cz = cn[kFZigZag[q]];   // lane z holds zig-zag index z of the NOMV residual
  uint64_t m = __ballot(abs(cz << 1) >= (int)a.floor[(3 + p) * 64 + q]);
  bool nz = false;
  while (m) {
    const int z = __builtin_ctzll(m);
    m &= m - 1;
    const int c = __shfl(cz, z);
    nz |= rate_quant(c, a.tab[((3 + p) * 64 + z) * 64 + q]) != 0;
  }
  const bool isc = s.mode != kEncPixNomv || nz;
  const uint64_t bc = __ballot(isc), bp = __ballot(s.mode != kEncPixIntra);
  if (q == 0) {
    coded[fi] = bc;
    cls[fi] = bp;
  }
}

// token t (spec 7.7) counted for lane q: bin (chroma, Huffman group of its start index z, t) of the u16-pair histogram
__device__ __forceinline__ void rate_count(uint32_t *h, int cc, int z, int t) {
  const int hg = z == 0 ? 0 : z <= 5 ? 1 : z <= 14 ? 2 : z <= 27 ? 3 : 4;
  const int i = (cc * 5 + hg) * 32 + t;
  atomicAdd(&h[i >> 1], 1u << (16 * (i & 1)));
}

// grid: nwg persistent work groups of kRateTokWaves waves; wave w of work group wg takes the blocks wg * 16 + w + k * 16 nwg (nwg
// from rate_groups, or a caller's count below kRateBlocksPerGroupLimit blocks a group: see kRateMaxBlocksPerGroup).  partial [nwg][64][kRatePartial] u32: the work group's
// token histogram per q, then (inter) its side count 3 M + 12 V
template <bool kInter>
__global__ __launch_bounds__(64 * kRateTokWaves) void k_rate_tok(uint32_t *partial, const int16_t *qdc, const uint64_t *coded, const uint64_t *cls,
                                                  RateArgs a, EncPlanes g, int64_t nfrags) {
  constexpr int kTabs = kInter ? 6 : 3;
  __shared__ uint32_t s_h[64 * kRateHistStride];
  __shared__ uint32_t s_side[64];
  // the quantiser entries (d | m << 16) of the tables this frame type uses, [table][z][q]: lane q reads a word of its own bank.
  // (Read from global memory, every index a lane quantises cost a dependent round trip.)  l follows from d (rate_entry).  s_floor:
  // the least step over q of each (table, z), for the ballot of the indices any q may find non-zero -- the minimum of the row's 64
  // entries in s_tab, one thread a row.  Thread i starts at entry i & 63, so that the lanes of a wave, whose rows lie 64 words
  // apart, read 64 different banks.
  __shared__ uint32_t s_tab[kTabs * 64 * 64];
  __shared__ uint32_t s_floor[kTabs * 64];
  for (int i = (int)threadIdx.x; i < 64 * kRateHistStride; i += 64 * kRateTokWaves) s_h[i] = 0;
  for (int i = (int)threadIdx.x; i < kTabs * 64 * 64; i += 64 * kRateTokWaves) s_tab[i] = a.tab[i].x;
  if (threadIdx.x < 64) s_side[threadIdx.x] = 0;
  __syncthreads();
  for (int i = (int)threadIdx.x; i < kTabs * 64; i += 64 * kRateTokWaves) {
    uint32_t m = 0xFFFFu;
#pragma unroll 8
    for (int k = 0; k < 64; k++) m = min(m, s_tab[i * 64 + ((k + i) & 63)] & 0xFFFFu);
    s_floor[i] = m;
  }
  __syncthreads();
  const int q = (int)threadIdx.x & 63;
  uint32_t *h = s_h + q * kRateHistStride;
  const int64_t step = (int64_t)gridDim.x * kRateTokWaves;
  for (int64_t fi = (int64_t)blockIdx.x * kRateTokWaves + (threadIdx.x >> 6); fi < nfrags; fi += step) {
    int p, fx, fy;
    enc_frag_xy(g, (int)fi, p, fx, fy);
    const int nh = g.nh[p];
    const RateSel s = rate_select<kInter>(a.mbs, a.lam, p, fx, fy, a.hdec, a.vdec, a.nmbx, q);
    const bool isc = kInter ? ((coded[fi] >> q) & 1ull) != 0 : true;
    // DC: spec 7.8 from the neighbours coded at q in the block's class (inter: no "last DC" fallback, the predictor is then 0)
    const uint64_t bit = 1ull << q;
    const uint64_t mycls = kInter ? cls[fi] & bit : 0;
    auto same = [&](int64_t f) { return !kInter || ((coded[f] & bit) && (cls[f] & bit) == mycls); };
    int l = 0, ul = 0, u = 0, ur = 0, msk = 0;
    if (fx > 0 && same(fi - 1)) { l = qdc[(fi - 1) * 64 + q]; msk |= 1; }
    if (fy > 0) {
      if (fx > 0 && same(fi - nh - 1)) { ul = qdc[(fi - nh - 1) * 64 + q]; msk |= 2; }
      if (same(fi - nh)) { u = qdc[(fi - nh) * 64 + q]; msk |= 4; }
      if (fx + 1 < nh && same(fi - nh + 1)) { ur = qdc[(fi - nh + 1) * 64 + q]; msk |= 8; }
    }
    const int dc = (int)qdc[fi * 64 + q] - enc_dc_pred(msk, l, ul, u, ur);
    // lane z holds zig-zag index z of each residual the block may code; the indices any q may find non-zero
    const int nvar = kInter ? 3 : 1;
    int cz[3] = {0, 0, 0};
    uint64_t any = 0;
    for (int v = 0; v < nvar; v++) {
      cz[v] = a.coef[((int64_t)v * nfrags + fi) * 64 + kFZigZag[q]];
      const int t = v == 0 ? p : 3 + p;
      any |= __ballot(abs(cz[v] << 1) >= (int)s_floor[t * 64 + q]);
    }
    any &= ~1ull;
    const int cc = p > 0;
    int next = 0;
    auto emit_value = [&](int v, int z) {   // v != 0 after `next`: the tokens of enc_block_tokens
      const int gap = z - next, av = abs(v);
      if (av == 1 && gap >= 1 && gap <= 17) {
        rate_count(h, cc, next, gap <= 5 ? 22 + gap : gap <= 9 ? 28 : 29);
      } else if ((av == 2 || av == 3) && gap >= 1 && gap <= 3) {
        rate_count(h, cc, next, gap == 1 ? 30 : 31);
      } else {
        if (gap > 0) rate_count(h, cc, next, gap <= 8 ? 7 : 8);
        int t, x;
        enc_value_token(v, t, x);
        rate_count(h, cc, z, t);
      }
      next = z + 1;
    };
    if (isc && dc) emit_value(dc, 0);
    while (any) {
      const int z = __builtin_ctzll(any);
      any &= any - 1;
      const int c0 = __shfl(cz[0], z);
      const int c1 = kInter ? __shfl(cz[1], z) : 0, c2 = kInter ? __shfl(cz[2], z) : 0;
      const int lv = rate_quant(s.var == 0 ? c0 : s.var == 1 ? c1 : c2, rate_entry(s_tab[(s.tab * 64 + z) * 64 + q]));
      if (isc && lv) emit_value(lv, z);
    }
    if (isc && next < 64) rate_count(h, cc, next, 0);   // the block's own EOB
    if (kInter && p == 0 && !(fx & 1) && !(fy & 1)) {
      // the macro block's side bits: 3 for its mode, 12 more for a vector, when one of its four luma blocks is coded
      const uint64_t mc = coded[fi] | coded[fi + 1] | coded[fi + nh] | coded[fi + nh + 1];
      if ((mc >> q) & 1ull) atomicAdd(&s_side[q], s.mode == kEncPixMv ? 15u : 3u);
    }
  }
  __syncthreads();
  uint32_t *out = partial + (int64_t)blockIdx.x * 64 * kRatePartial;
  for (int i = (int)threadIdx.x; i < 64 * kRateBins; i += 64 * kRateTokWaves) {
    const int qq = i / kRateBins, bin = i - qq * kRateBins;
    out[qq * kRatePartial + bin] = (s_h[qq * kRateHistStride + (bin >> 1)] >> (16 * (bin & 1))) & 0xFFFFu;
  }
  if (threadIdx.x < 64) out[threadIdx.x * kRatePartial + kRateBins] = s_side[threadIdx.x];
}

// extra bits after each DCT token (spec Tables 7.33 / 7.38)
__device__ constexpr uint8_t kRateExtraBits[32] = {0, 0, 0, 2, 3, 4, 12, 3, 6, 0, 0, 0, 0, 1, 1, 1,
                                                   1, 2, 3, 4, 5, 6, 10, 1, 1, 1, 1, 1, 3, 4, 2, 3};

// grid: 64 work groups of 1024 threads, one per q.  lens [80][32]: the setup's code lengths.  est [64] int64: E[q].  fixed: header bits (and, inter,
// nfrags / 8)
__global__ __launch_bounds__(1024) void k_rate_bits(int64_t *est, const uint32_t *partial, int nwg, const uint8_t *lens, int fixed) {
  __shared__ uint32_t s_h[kRatePartial];
  __shared__ uint64_t s_cost[64];
  const int q = (int)blockIdx.x;
  for (int i = (int)threadIdx.x; i < kRatePartial; i += 1024) s_h[i] = 0;
  __syncthreads();
  // the partials' rows of q, flattened: every thread's loads are independent of each other (no chain of nwg loads)
  const int total = nwg * kRatePartial;
#pragma unroll 4
  for (int k = (int)threadIdx.x; k < total; k += 1024) {
    const int w = k / kRatePartial, i = k - w * kRatePartial;
    const uint32_t v = partial[((int64_t)w * 64 + q) * kRatePartial + i];
    if (v) atomicAdd(&s_h[i], v);
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // choice c (DC luma, DC chroma, AC luma, AC chroma), table t
    const int c = (int)threadIdx.x >> 4, t = (int)threadIdx.x & 15, ac = c >> 1, cc = c & 1;
    uint64_t bits = 0;
    for (int hg = ac ? 1 : 0; hg < (ac ? 5 : 1); hg++)
      for (int tok = 0; tok < 32; tok++) bits += (uint64_t)s_h[(cc * 5 + hg) * 32 + tok] * lens[(16 * hg + t) * 32 + tok];
    s_cost[threadIdx.x] = bits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t e = (uint64_t)fixed + s_h[kRateBins];
    for (int c = 0; c < 4; c++) {
      uint64_t best = s_cost[c * 16];
      for (int t = 1; t < 16; t++) best = s_cost[c * 16 + t] < best ? s_cost[c * 16 + t] : best;
      e += best;
    }
    for (int i = 0; i < kRateBins; i++) e += (uint64_t)s_h[i] * kRateExtraBits[i & 31];
    est[q] = (int64_t)e;
  }
}

// ---- the launches, the table and the grid rule, stated once: the probe (enc_rate_probe, thip_encode.hip) and thip_enc_rate_stage
// (theora_hip.h) both call these ---------------------------------------------------------------------------------------------------

// k_rate_tok's work groups for nfrags blocks: one wave a block up to 256 groups, then as many as keep a group's blocks at or below
// kRateMaxBlocksPerGroup + kRateTokWaves (a group takes at most ceil(nfrags / groups) + kRateTokWaves blocks)
inline int rate_groups(int64_t nfrags) {
  const int64_t rounds = (nfrags + kRateTokWaves - 1) / kRateTokWaves, a = rounds < 256 ? rounds : 256;
  const int64_t b = (nfrags + kRateMaxBlocksPerGroup - 1) / kRateMaxBlocksPerGroup;
  return (int)(a > b ? a : b);
}
constexpr int64_t kRateMaxFrags = (int64_t)1 << 24;

// the blocks the busiest work group of `groups` takes: its 16 waves take a block each per round
inline int64_t rate_blocks_per_group(int64_t nfrags, int groups) {
  const int64_t rounds = (nfrags + kRateTokWaves - 1) / kRateTokWaves;
  return (rounds + groups - 1) / groups * kRateTokWaves;
}

// oc_enc_quantize's table entries of every (table, z, q) from the steps [6][64 q][64 z] (zig-zag; intra then inter per plane), as
// k_enc_intra_fq forms them: (step | m << 16, l).  rate_quant reads the second word as l alone: no zig-zag index in it.
inline void rate_form_table(uint2 *tab, const uint16_t *steps) {
  for (int t = 0; t < 6; t++)
    for (int q = 0; q < 64; q++)
      for (int z = 0; z < 64; z++) tab[(t * 64 + z) * 64 + q] = enc_quant_entry(steps[(t * 64 + q) * 64 + z], 0);
}

// (rate_steps_ok, what the probe asks of a table set, and rate_form_floor are host arithmetic: thip_quant.h)

// coef [1 or 3][nfrags][64]; R, mbs: the inter frame's reference and k_rate_me's words
inline hipError_t rate_launch_coef(int16_t *coef, const EncPlanes &g, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_rate_fdct_key, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, stream, coef, g, n);
  return hipGetLastError();
}
inline hipError_t rate_launch_coef(int16_t *coef, const EncPlanes &g, const EncRef &R, const uint4 *mbs, int nmbx, int64_t n,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(k_rate_fdct_inter, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, stream, coef, g, R, mbs, nmbx, n);
  return hipGetLastError();
}

inline hipError_t rate_launch_dc(bool inter, int16_t *qdc, uint64_t *coded, uint64_t *cls, const RateArgs &a, const EncPlanes &g,
                                 int64_t n, hipStream_t stream) {
  const dim3 grid((unsigned)((n + 3) / 4));
  if (inter) hipLaunchKernelGGL(k_rate_dc<true>, grid, dim3(256), 0, stream, qdc, coded, cls, a, g, n);
  else hipLaunchKernelGGL(k_rate_dc<false>, grid, dim3(256), 0, stream, qdc, coded, cls, a, g, n);
  return hipGetLastError();
}

inline hipError_t rate_launch_tok(bool inter, uint32_t *partial, int groups, const int16_t *qdc, const uint64_t *coded,
                                  const uint64_t *cls, const RateArgs &a, const EncPlanes &g, int64_t n, hipStream_t stream) {
  const dim3 grid((unsigned)groups), block(64 * kRateTokWaves);
  if (inter) hipLaunchKernelGGL(k_rate_tok<true>, grid, block, 0, stream, partial, qdc, coded, cls, a, g, n);
  else hipLaunchKernelGGL(k_rate_tok<false>, grid, block, 0, stream, partial, qdc, coded, cls, a, g, n);
  return hipGetLastError();
}

inline hipError_t rate_launch_bits(int64_t *est, const uint32_t *partial, int groups, const uint8_t *lens, int fixed,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(k_rate_bits, dim3(64), dim3(1024), 0, stream, est, partial, groups, lens, fixed);
  return hipGetLastError();
}

}  // namespace thip
