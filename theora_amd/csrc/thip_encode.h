// thip_encode.h -- the device stage of the intra-only th_encode_* encoder (thip_encode.hip): four launches a frame, none of which
// waits for another on the host.
//
// The pieces of k_enc_intra_fq -- the quantiser tables (enc_quant_tables), a lane's two rows into LDS (enc_stage_rows), what
// follows the quantiser (enc_fq_tail) -- are functions here: the inter, all-modes, block-qi and rate-probe kernels
// (thip_encode_inter.h, thip_encode_modes.h, thip_encode_bqi.h, thip_rate.h) are made of the same ones.  The transform, the
// quantiser and the LDS layout between them are thip_fdct.h's, the same code as the batched slots run.
//
//   k_enc_intra_fq       transform and quantise.  Four lanes a block (fdct_quantize4_lds of thip_fdct.h): each lane loads two
//                        rows of its block straight from the caller's planes (any stride or
//                        alignment; coordinates clamped to the picture region), subtracts 128, and the block goes through the fDCT
//                        and the quantiser of its plane.  Out: the zig-zag levels of block k (coded order) at levels[64 k], the
//                        quantised DC by raster fragment index at dcq[fi].
//   k_enc_intra_tok      forward DC prediction and tokenisation, one lane a block.  In an intra frame every fragment is coded from
//                        the same reference, so a block's predictor (spec 7.8) needs nothing but its neighbours' quantised DCs:
//                        one parallel pass.  Out: the block's tokens as words (below) at tok[kEncTokWords k], a 64-bit mask of
//                        the zig-zag indices at which its tokens start (at most one a block and index), and the work group's
//                        token count per (plane, index).
//   k_enc_intra_scan     one work group per zig-zag index: the exclusive scan of the groups' counts (chunk_base) and the lengths of
//                        the 64 x 3 token lists.
//   k_enc_intra_scatter  each block's tokens to their place in stream order (spec 7.7.3: index, then plane, then coded order), EOB
//                        runs not yet merged -- the host does that, then the Huffman tables and the bits.
//
// Token word: token (5 bits) | extra bits << 5 (up to 10 of them; how many follows from the token) | zig-zag index << 16 |
// plane << 22.  A block's EOB is token 0 (a run of one); the host merges runs of them.
#pragma once
#include "thip_fdct.h"

namespace thip {

constexpr int kEncTokWords = 65;   // worst case a block: 64 value tokens and an EOB
constexpr int kEncChunk = 256;     // blocks a work group of k_enc_intra_tok / k_enc_intra_scatter

struct EncPlanes {
  const uint8_t *src[3];   // the picture's top-left pixel in each plane
  int64_t stride[3];       // bytes from one row to the next one down
  int px0[3], py0[3];      // the picture's top-left in the plane (rows counted from the top)
  int pw[3], ph[3];        // the picture's size in the plane
  int nh[3], nv[3], froff[3];
};

__device__ __forceinline__ int enc_plane_of(const EncPlanes &g, int fi) { return fi >= g.froff[2] ? 2 : fi >= g.froff[1] ? 1 : 0; }

// the raster fragment fi's plane, column, row (rows from the bottom)
__device__ __forceinline__ void enc_frag_xy(const EncPlanes &g, int fi, int &p, int &fx, int &fy) {
  p = enc_plane_of(g, fi);
  const int loc = fi - g.froff[p];
  fy = loc / g.nh[p];
  fx = loc - fy * g.nh[p];
}

// ---- the pieces every transform-and-quantise kernel is made of (k_enc_intra_fq here, enc_inter_fq of thip_encode_inter.h,
// enc_fq_bqi of thip_encode_bqi.h, the probe's transforms of thip_rate.h).  Four lanes a block, sixteen blocks a wave: lane
// 4 b + j holds rows 2j, 2j + 1 of block b; the wave's 128 int4 of LDS hold row r of block b at lds_block_piece(b, r).

// the table entry (quant_entry of thip_fdct.h) of the step dq at zig-zag index z, its reciprocal derived (quant_recip)
__host__ __device__ __forceinline__ uint2 enc_quant_entry(uint32_t dq, int z) {
  int m, l;
  quant_recip(dq << 1, m, l);
  return quant_entry(dq, m, l, z);
}

// `ntabs` tables of `dequant` ([ntabs][64], zig-zag) as entries by natural position in s_t, by the whole work group
__device__ __forceinline__ void enc_quant_tables(uint2 *s_t, const uint16_t *dequant, int ntabs) {
  for (int i = (int)threadIdx.x; i < ntabs * 64; i += 256) {
    const int z = i & 63;
    s_t[(i & ~63) + kFZigZag[z]] = enc_quant_entry(dequant[i], z);
  }
}

// The source pixels of block (p, fx, fy), the picture clamped outward: the plane's scalars by value and the clamped columns, once
// for all the block's rows (chosen a pixel at a time, the plane's members and the clamps are recomputed a pixel at a time)
struct EncSrcBlock {
  const uint8_t *src;
  int64_t stride;
  int top, ph1;   // block row r (from the BOTTOM, spec 2.2) is picture row top - r, clamped to [0, ph1]
  int cx[8];
};
__device__ __forceinline__ EncSrcBlock enc_src_block(const EncPlanes &g, int p, int fx, int fy) {
  EncSrcBlock s;
  s.src = g.src[p];
  s.stride = g.stride[p];
  s.top = g.nv[p] * 8 - 1 - fy * 8 - g.py0[p];
  s.ph1 = g.ph[p] - 1;
  const int x0 = fx * 8 - g.px0[p], pw1 = g.pw[p] - 1;
#pragma unroll
  for (int c = 0; c < 8; c++) s.cx[c] = min(max(x0 + c, 0), pw1);
  return s;
}
__device__ __forceinline__ const uint8_t *enc_src_row(const EncSrcBlock &s, int r) {
  return s.src + (int64_t)min(max(s.top - r, 0), s.ph1) * s.stride;
}

// a lane's two rows of its block into the wave's LDS as packed int16; row(r, v) fills v[0..7] with row r of the residual (rows from
// the bottom).  A lane past the last block (!live) stores zeros.
template <class Row>
__device__ __forceinline__ void enc_stage_rows(int4 *lds, int b, int j, bool live, Row &&row) {
  if (live) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = 2 * j + h;
      int v[8];
      row(r, v);
      lds[lds_block_piece(b, r)] = make_int4((v[0] & 0xFFFF) | (v[1] << 16), (v[2] & 0xFFFF) | (v[3] << 16),
                                             (v[4] & 0xFFFF) | (v[5] << 16), (v[6] & 0xFFFF) | (v[7] << 16));
    }
  } else {
    lds[lds_block_piece(b, 2 * j)] = make_int4(0, 0, 0, 0);
    lds[lds_block_piece(b, 2 * j + 1)] = make_int4(0, 0, 0, 0);
  }
}

enum { kEncPixNomv = 0, kEncPixIntra = 1, kEncPixMv = 2, kEncPixGoldNomv = 5, kEncPixGoldMv = 6, kEncPixFour = 7 };   // (the spec's mode numbers)
__device__ __forceinline__ bool enc_pix_gold(int pix) { return pix == kEncPixGoldNomv || pix == kEncPixGoldMv; }

// What follows the quantiser.  The wave's levels go out (block b0 + bb from src(bb), the lane's own block's are `own`: the wave's
// LDS, or the block's chosen qi), the
// quantised DC of the lane's block (zig-zag index 0 in `lds`) to dcq[fi], and with kClasses reference classes (2: intra, PREV; 3:
// GOLD too; 0: a key frame, nothing more) the block's coded flag and class to cmap[fi] -- an INTRA or MV block is always coded, a
// NOMV one when a level is not zero -- and the last coded fragment (+1) of its 256 raster fragments and class to dclast.
template <int kClasses, class Src>
__device__ __forceinline__ void enc_fq_tail(int16_t *levels, int16_t *dcq, uint8_t *cmap, uint32_t *dclast, const int4 *lds,
                                            Src &&src, const int4 *own, int64_t b0, int64_t n, int fi, int pix) {
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  wave_blocks_out_of(levels, src, b0, n);
  const bool first = j == 0 && b0 + b < n;   // the lane that writes for its block
  if constexpr (kClasses == 0) {
    if (first) dcq[fi] = (int16_t)lds[lds_block_piece(b, 0)].x;
  } else {
    // any level of the block not zero: lane j looks at rows 2j, 2j + 1 of its (rotated) zig-zag pieces
    const int4 r0 = own[lds_block_piece(b, 2 * j)], r1 = own[lds_block_piece(b, 2 * j + 1)];
    int nz = (r0.x | r0.y | r0.z | r0.w | r1.x | r1.y | r1.z | r1.w) != 0;
    nz |= __shfl_xor(nz, 1);
    nz |= __shfl_xor(nz, 2);
    if (!first) return;
    dcq[fi] = (int16_t)lds[lds_block_piece(b, 0)].x;
    const int cls = pix == kEncPixIntra ? 1 : kClasses == 3 && enc_pix_gold(pix) ? 3 : 2;
    const bool coded = pix != kEncPixNomv || nz;
    cmap[fi] = coded ? (uint8_t)cls : (uint8_t)0;
    if (coded) atomicMax(&dclast[(fi >> 8) * kClasses + cls - 1], (uint32_t)fi + 1u);
  }
}

// levels [n][64] int16 (zig-zag), dcq [nfrags] int16 (raster), overflow: zeroed for k_enc_intra_tok, dequant [3][64] (zig-zag, the intra tables of the frame's qi)
__global__ __launch_bounds__(256) void k_enc_intra_fq(int16_t *levels, int16_t *dcq, uint32_t *overflow, const int32_t *coded_order,
                                                      EncPlanes g, const uint16_t *dequant, int64_t n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;   // (k_enc_intra_tok counts into it)
  __shared__ __attribute__((aligned(16))) uint2 s_t[3 * 64];   // per plane, by natural position (see fdct_quantize4_lds)
  enc_quant_tables(s_t, dequant, 3);
  __shared__ int4 s_x[4 * 128];
  int4 *lds = s_x + (threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t b0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2;
  const int64_t k = b0 + b;
  const int fi = coded_order[min(k, n - 1)];   // (a lane past the last block: any block's, it stores nothing)
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  enc_stage_rows(lds, b, j, k < n, [&](int r, int v[8]) {
    const uint8_t *row = enc_src_row(sb, r);
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = (int)row[sb.cx[c]] - 128;
  });
  __syncthreads();   // (the tables too)
  fdct_quantize4_lds(lds, s_t + 64 * p, b, j);
  enc_fq_tail<0>(levels, dcq, nullptr, nullptr, lds, [=](int) { return lds; }, lds, b0, n, fi, kEncPixIntra);
}

// the smallest value token of a coefficient (spec Table 7.38); false when |v| > 580
__device__ __forceinline__ bool enc_value_token(int v, int &tok, int &extra) {
  const int a = abs(v), s = v < 0 ? 1 : 0;
  if (a == 1) { tok = 9 + s; extra = 0; }
  else if (a == 2) { tok = 11 + s; extra = 0; }
  else if (a <= 6) { tok = 10 + a; extra = s; }
  else if (a <= 8) { tok = 17; extra = s << 1 | (a - 7); }
  else if (a <= 12) { tok = 18; extra = s << 2 | (a - 9); }
  else if (a <= 20) { tok = 19; extra = s << 3 | (a - 13); }
  else if (a <= 36) { tok = 20; extra = s << 4 | (a - 21); }
  else if (a <= 68) { tok = 21; extra = s << 5 | (a - 37); }
  else if (a <= 580) { tok = 22; extra = s << 9 | (a - 69); }
  else { tok = 22; extra = s << 9 | 511; return false; }
  return true;
}

// The DC predictor and the tokens of k_enc_intra_tok as functions, for k_enc_inter_tok / k_enc_inter_dc (thip_encode_inter.h).
// k_enc_intra_tok keeps its inline copy: calling these from it changed its resource line.
//
// spec 7.8 (decode.c:1450-1485) from the neighbour mask (1 left, 2 upper-left, 4 upper, 8 upper-right) and the neighbours' quantised
// DCs; mask 0 gives 0 (the caller's own fallback)
__device__ __forceinline__ int enc_dc_pred(int msk, int l, int ul, int u, int ur) {
  int pred = 0;
  switch (msk) {
    case 1: case 3: pred = l; break;
    case 2: pred = ul; break;
    case 4: case 6: case 12: pred = u; break;
    case 5: pred = (l + u) / 2; break;
    case 8: pred = ur; break;
    case 9: case 11: case 13: pred = (75 * l + 53 * ur) / 128; break;
    case 10: pred = (ul + ur) / 2; break;
    case 14: pred = (3 * (ul + ur) + 10 * u) / 16; break;
    case 7: case 15:
      pred = (29 * (l + u) - 26 * ul) / 32;
      if (abs(pred - u) > 128) pred = u;
      else if (abs(pred - l) > 128) pred = l;
      else if (abs(pred - ul) > 128) pred = ul;
      break;
    default: break;
  }
  return pred;
}

// the tokens of the non-zero value a at zig-zag index z when the block's previous token ended before index `next` (spec 7.7.1): a
// combined token if one fits, else a zero run (when z > next) and the smallest value token.  emit(token, extra, start index) for
// each; returns the number of overflows (0 or 1).  The block-qi choice (thip_encode_bqi.h) counts with it.  enc_block_tokens below
// keeps its inline form of the same rule: calling this function from it cost k_enc_inter_tok's resource line a VGPR.
template <class Emit>
__device__ __forceinline__ int enc_value_tokens(int a, int z, int next, Emit &&emit) {
  const int gap = z - next, aa = abs(a), s = a < 0 ? 1 : 0;
  if (aa == 1 && gap >= 1 && gap <= 17) {   // RUN_CAT1A / B / C
    if (gap <= 5) emit(22 + gap, s, next);
    else if (gap <= 9) emit(28, s << 2 | (gap - 6), next);
    else emit(29, s << 3 | (gap - 10), next);
  } else if ((aa == 2 || aa == 3) && gap >= 1 && gap <= 3) {   // RUN_CAT2A / B
    if (gap == 1) emit(30, s << 1 | (aa - 2), next);
    else emit(31, s << 2 | (aa - 2) << 1 | (gap - 2), next);
  } else {
    if (gap > 0) {
      if (gap <= 8) emit(7, gap - 1, next);   // SHORT_ZRL
      else emit(8, gap - 1, next);            // ZRL
    }
    int t, extra;
    const int ovf = enc_value_token(a, t, extra) ? 0 : 1;
    emit(t, extra, z);
    return ovf;
  }
  return 0;
}

// the tokens of one block (zig-zag levels lv, its DC residual dc, plane p) as words at out, the indices at which they start in m,
// counted per (plane, index) in s_cnt; returns the number of overflows
__device__ __forceinline__ int enc_block_tokens(uint32_t *out, uint64_t &mask_out, uint32_t *s_cnt, const int16_t *lv, int dc, int p) {
  // which levels are non-zero (the DC: its residual), then the tokens walk the non-zero ones in zig-zag order
  const int4 *src = reinterpret_cast<const int4 *>(lv);
  uint64_t nzm = 0;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int4 w = src[r];
    const int w4[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      nzm |= (uint64_t)((w4[q] & 0xFFFF) != 0) << (r * 8 + 2 * q);
      nzm |= (uint64_t)((w4[q] >> 16) != 0) << (r * 8 + 2 * q + 1);
    }
  }
  nzm = (nzm & ~1ull) | (uint64_t)(dc != 0);
  const uint32_t plane = (uint32_t)p << 22;
  uint64_t m = 0;
  int cnt = 0, ovf = 0, next = 0;   // next: the index after the last non-zero level written
  auto emit = [&](int t, int extra, int z) {
    out[cnt++] = (uint32_t)t | (uint32_t)extra << 5 | (uint32_t)z << 16 | plane;
    m |= 1ull << z;
    atomicAdd(&s_cnt[p * 64 + z], 1u);
  };
  while (nzm) {
    const int z = __builtin_ctzll(nzm);
    nzm &= nzm - 1;
    const int a = z ? (int)lv[z] : dc, gap = z - next;
    const int aa = abs(a), s = a < 0 ? 1 : 0;
    if (aa == 1 && gap >= 1 && gap <= 17) {   // RUN_CAT1A / B / C
      if (gap <= 5) emit(22 + gap, s, next);
      else if (gap <= 9) emit(28, s << 2 | (gap - 6), next);
      else emit(29, s << 3 | (gap - 10), next);
    } else if ((aa == 2 || aa == 3) && gap >= 1 && gap <= 3) {   // RUN_CAT2A / B
      if (gap == 1) emit(30, s << 1 | (aa - 2), next);
      else emit(31, s << 2 | (aa - 2) << 1 | (gap - 2), next);
    } else {
      if (gap > 0) {
        if (gap <= 8) emit(7, gap - 1, next);   // SHORT_ZRL
        else emit(8, gap - 1, next);            // ZRL
      }
      int t, extra;
      ovf += enc_value_token(a, t, extra) ? 0 : 1;
      emit(t, extra, z);
    }
    next = z + 1;
  }
  if (next < 64) emit(0, 0, next);   // EOB (a run of one; the host merges them)
  mask_out = m;
  return ovf;
}

// tok [n][kEncTokWords], mask [n], chunk_cnt [gridDim.x][3][64], overflow: one word
__global__ __launch_bounds__(256) void k_enc_intra_tok(uint32_t *tok, uint64_t *mask, uint32_t *chunk_cnt, uint32_t *overflow,
                                                       const int16_t *levels, const int16_t *dcq, const int32_t *coded_order,
                                                       EncPlanes g, int64_t n) {
  __shared__ uint32_t s_cnt[3 * 64];
  if (threadIdx.x < 192) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    const int fi = coded_order[k], p = enc_plane_of(g, fi), nh = g.nh[p];
    const int loc = fi - g.froff[p], fy = loc / nh, fx = loc - fy * nh;
    // spec 7.8 (decode.c:1450-1485) on the quantised DCs; every neighbour is coded from the same reference in an intra frame
    int l = 0, ul = 0, u = 0, ur = 0, msk = 0;
    if (fx > 0) { l = dcq[fi - 1]; msk |= 1; }
    if (fy > 0) {
      if (fx > 0) { ul = dcq[fi - nh - 1]; msk |= 2; }
      u = dcq[fi - nh];
      msk |= 4;
      if (fx + 1 < nh) { ur = dcq[fi - nh + 1]; msk |= 8; }
    }
    int pred = 0;   // mask 0: the plane's first fragment, pred_last = 0
    switch (msk) {
      case 1: case 3: pred = l; break;
      case 2: pred = ul; break;
      case 4: case 6: case 12: pred = u; break;
      case 5: pred = (l + u) / 2; break;
      case 8: pred = ur; break;
      case 9: case 11: case 13: pred = (75 * l + 53 * ur) / 128; break;
      case 10: pred = (ul + ur) / 2; break;
      case 14: pred = (3 * (ul + ur) + 10 * u) / 16; break;
      case 7: case 15:
        pred = (29 * (l + u) - 26 * ul) / 32;
        if (abs(pred - u) > 128) pred = u;
        else if (abs(pred - l) > 128) pred = l;
        else if (abs(pred - ul) > 128) pred = ul;
        break;
      default: break;
    }
    // which levels are non-zero (the DC: its residual), then the tokens walk the non-zero ones in zig-zag order
    const int16_t *lv = levels + k * 64;
    const int4 *src = reinterpret_cast<const int4 *>(lv);
    uint64_t nzm = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int4 w = src[r];
      const int w4[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        nzm |= (uint64_t)((w4[q] & 0xFFFF) != 0) << (r * 8 + 2 * q);
        nzm |= (uint64_t)((w4[q] >> 16) != 0) << (r * 8 + 2 * q + 1);
      }
    }
    const int dc = (int)lv[0] - pred;
    nzm = (nzm & ~1ull) | (uint64_t)(dc != 0);
    uint32_t *out = tok + k * kEncTokWords;
    const uint32_t plane = (uint32_t)p << 22;
    uint64_t m = 0;
    int cnt = 0, ovf = 0, next = 0;   // next: the index after the last non-zero level written
    auto emit = [&](int t, int extra, int z) {
      out[cnt++] = (uint32_t)t | (uint32_t)extra << 5 | (uint32_t)z << 16 | plane;
      m |= 1ull << z;
      atomicAdd(&s_cnt[p * 64 + z], 1u);
    };
    while (nzm) {
      const int z = __builtin_ctzll(nzm);
      nzm &= nzm - 1;
      const int a = z ? (int)lv[z] : dc, gap = z - next;
      const int aa = abs(a), s = a < 0 ? 1 : 0;
      if (aa == 1 && gap >= 1 && gap <= 17) {   // RUN_CAT1A / B / C
        if (gap <= 5) emit(22 + gap, s, next);
        else if (gap <= 9) emit(28, s << 2 | (gap - 6), next);
        else emit(29, s << 3 | (gap - 10), next);
      } else if ((aa == 2 || aa == 3) && gap >= 1 && gap <= 3) {   // RUN_CAT2A / B
        if (gap == 1) emit(30, s << 1 | (aa - 2), next);
        else emit(31, s << 2 | (aa - 2) << 1 | (gap - 2), next);
      } else {
        if (gap > 0) {
          if (gap <= 8) emit(7, gap - 1, next);   // SHORT_ZRL
          else emit(8, gap - 1, next);            // ZRL
        }
        int t, extra;
        ovf += enc_value_token(a, t, extra) ? 0 : 1;
        emit(t, extra, z);
      }
      next = z + 1;
    }
    if (next < 64) emit(0, 0, next);   // EOB (a run of one; the host merges them)
    mask[k] = m;
    if (ovf) atomicAdd(overflow, (uint32_t)ovf);
  }
  __syncthreads();
  if (threadIdx.x < 192) chunk_cnt[(int64_t)blockIdx.x * 192 + threadIdx.x] = s_cnt[threadIdx.x];
}

// exclusive prefix sum over the 256 threads of a work group (s_w: 4 words of LDS); returns the sum of all
__device__ __forceinline__ uint32_t enc_block_scan(uint32_t v, uint32_t &excl, uint32_t *s_w) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t c = s_w[q];
    before += q < w ? c : 0u;
    total += c;
  }
  __syncthreads();
  excl = before + x - v;
  return total;
}

// grid: 64 work groups, one per zig-zag index.  chunk_base [nchunks][64], list_len [3][64]
__global__ __launch_bounds__(256) void k_enc_intra_scan(uint32_t *chunk_base, uint32_t *list_len, const uint32_t *chunk_cnt,
                                                        int nchunks) {
  __shared__ uint32_t s_w[4], s_pl[3];
  const int z = (int)blockIdx.x;
  if (threadIdx.x < 3) s_pl[threadIdx.x] = 0;
  uint32_t run = 0, pl[3] = {0, 0, 0};
  for (int c0 = 0; c0 < nchunks; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    uint32_t v = 0;
    if (c < nchunks) {
#pragma unroll
      for (int p = 0; p < 3; p++) {
        const uint32_t x = chunk_cnt[(int64_t)c * 192 + p * 64 + z];
        pl[p] += x;
        v += x;
      }
    }
    uint32_t excl;
    const uint32_t total = enc_block_scan(v, excl, s_w);
    if (c < nchunks) chunk_base[(int64_t)c * 64 + z] = run + excl;
    run += total;
  }
#pragma unroll
  for (int p = 0; p < 3; p++)
    if (pl[p]) atomicAdd(&s_pl[p], pl[p]);
  __syncthreads();
  if (threadIdx.x < 3) list_len[threadIdx.x * 64 + z] = s_pl[threadIdx.x];
}

// grid: the chunks of k_enc_intra_tok.  out: the frame's tokens in stream order
__global__ __launch_bounds__(256) void k_enc_intra_scatter(uint32_t *out, const uint32_t *tok, const uint64_t *mask,
                                                           const uint32_t *chunk_base, const uint32_t *list_len, int64_t n) {
  __shared__ uint32_t s_base[64], s_wcnt[4][64];
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  if (threadIdx.x < 64) {   // where the tokens of index z start: the lengths of all lists of lower indices
    const uint32_t tot = list_len[lane] + list_len[64 + lane] + list_len[128 + lane];
    uint32_t x = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    s_base[lane] = x - tot;
  }
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t m = k < n ? mask[k] : 0ull;
  for (int z = 0; z < 64; z++) {
    const uint64_t bal = __ballot((m >> z) & 1ull);
    if (lane == 0) s_wcnt[w][z] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint32_t *src = tok + k * kEncTokWords;
  int t = 0;
  for (int z = 0; z < 64; z++) {
    const bool has = (m >> z) & 1ull;
    const uint64_t bal = __ballot(has);
    if (has) {
      uint32_t off = s_base[z] + chunk_base[(int64_t)blockIdx.x * 64 + z] + (uint32_t)__popcll(bal & lt);
      for (int q = 0; q < w; q++) off += s_wcnt[q][z];
      out[off] = src[t++];
    }
  }
}

// ---- the launches, stated once: th_encode_* (thip_encode.hip) and thip_enc_tok_stage (theora_hip.h) both call these -------------
// The inter frame's token launch is tok_launch_inter of thip_encode_inter.h.
struct TokBufs {          // device memory a token launch writes
  uint32_t *tok;          // [n][kEncTokWords]: a block's tokens from its first word on, the words behind them untouched
  uint64_t *mask;         // [n]
  uint32_t *chunk_cnt;    // [enc_chunks(n)][3][64]
  uint32_t *overflow;     // one word, zeroed on the same stream before (the quantising kernels do)
};

inline unsigned enc_chunks(int64_t n) { return (unsigned)((n + kEncChunk - 1) / kEncChunk); }

// a key frame's tokens: levels [n][64] (coded order), dcq [n] (raster), order [n] (the coded order)
inline hipError_t tok_launch_intra(const TokBufs &o, const int16_t *levels, const int16_t *dcq, const int32_t *order, const EncPlanes &g,
                                   int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_intra_tok, dim3(enc_chunks(n)), dim3(256), 0, stream, o.tok, o.mask, o.chunk_cnt, o.overflow, levels, dcq,
                     order, g, n);
  return hipGetLastError();
}

// the chunks' counts into their places: chunk_base [enc_chunks(n)][64], list_len [3][64]
inline hipError_t tok_launch_scan(uint32_t *chunk_base, uint32_t *list_len, const uint32_t *chunk_cnt, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_intra_scan, dim3(64), dim3(256), 0, stream, chunk_base, list_len, chunk_cnt, (int)enc_chunks(n));
  return hipGetLastError();
}

// the blocks' tokens into stream order: out holds the sum of list_len words
inline hipError_t tok_launch_scatter(uint32_t *out, const uint32_t *tok, const uint64_t *mask, const uint32_t *chunk_base,
                                     const uint32_t *list_len, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_intra_scatter, dim3(enc_chunks(n)), dim3(256), 0, stream, out, tok, mask, chunk_base, list_len, n);
  return hipGetLastError();
}

}  // namespace thip
