// thip_encode_inter.h -- the device stage of an inter frame of th_encode_* (thip_encode.hip; the bitstream is stated in
// theoraenc_hip.h).  Everything is in bitstream coordinates: rows counted from the BOTTOM of the coded frame (spec 2.2), vectors
// in half pixels with y pointing up.  The reference is PREV, a frame of the encoder's own decoder: three planes, bitstream row order,
// no border (reads clamp their coordinates, as the decoder's motion-compensated reads do).  With all eight modes
// (thip_encode_modes.h) there is a second reference, GOLD; the bodies here are written once for both and the kernels are their
// named instances.
//
//   enc_me_search   the motion search of a macro block, one work group: the 48 x 48 reference window around it (the search range
//                   plus one pixel for the half-pel reads, coordinates clamped) and the 16 x 16 source go through LDS; a lane
//                   takes one full-pel candidate in four (961 of them: every (dx, dy) in [-15, 15]^2), a row costs four v_sad_u8
//                   on alignbyte-shifted words.  The best full-pel vector is refined over its eight half-pel neighbours with the
//                   decoder's own prediction (mv_axis, a truncating average of two reads).  Thread 0 gets S0, Smv, SI and the vector.
//   k_enc_me        enc_me_search, then the decision.  Out: one word a macro block (raster order, rows from the bottom): the pixel
//                   mode (NOMV / INTRA / MV) | mvx << 8 | mvy << 16 (bytes, zero unless MV).  (k_rate_me of thip_rate.h writes the
//                   statistics instead.)
//   enc_block_pred  a block's prediction from its macro block's word (k_enc_me's or k_enc_me_all's): pixel mode, vector (with the
//                   chroma vector of spec 7.9.4 for 4:2:0 and 4:2:2), reference plane.  enc_pred_block turns it into the block's read
//                   offsets and clamped columns once; enc_residual_row subtracts it from the source row by row (128 for INTRA).
//   k_enc_inter_fq  (enc_inter_fq over k_enc_me's words) k_enc_intra_fq for an inter frame: the prediction is subtracted, the block
//                   is transformed and quantised with the intra or inter table of its plane, and its coded flag is set
//                   (enc_fq_tail).  cmap[fi] (raster): 0 uncoded, 1 coded intra, 2 coded from PREV.
//   k_enc_inter_dc  (enc_inter_dc<2>) the DC residuals of spec 7.8 with reference classes: a neighbour counts when it is coded and
//                   of the same class; a block with none predicts from the last coded DC of its class before it in the plane's
//                   raster order -- a segmented "last value" scan (a max-scan of fragment indices, cut at the plane's first fragment).
//   k_enc_inter_tok k_enc_intra_tok over the coded blocks only (an uncoded block has no tokens and an empty mask), with the DC
//                   residual of k_enc_inter_dc.  k_enc_intra_scan and k_enc_intra_scatter then serve both frame types.
// The launches of the search, of k_enc_inter_fq and of k_enc_inter_dc are the launch functions at the end of this file (their
// eight-mode overloads: thip_encode_modes.h); th_encode_* and the test entry thip_enc_inter_stage (theora_hip.h) both call them.
#pragma once
#include "thip_encode.h"

namespace thip {

constexpr int kMeRange = 15;              // full-pel search: dx, dy in [-15, 15]
constexpr int kMeSide = 31;               // candidates a side
constexpr int kMeWin = 48;                // window side: 16 + 2 * (15 + 1)

struct EncRef {            // PREV or GOLD, bitstream row order
  const uint8_t *plane[3];
  int stride[3];
  int w[3], h[3];
  int hdec, vdec;
};

// the source pixel (x, y) of plane p, y counted from the bottom: the picture clamped outward, as k_enc_intra_fq reads it
__device__ __forceinline__ int enc_src_px(const EncPlanes &g, int p, int x, int y) {
  const int top = g.nv[p] * 8 - 1 - y;
  const int r = min(max(top - g.py0[p], 0), g.ph[p] - 1), c = min(max(x - g.px0[p], 0), g.pw[p] - 1);
  return (int)g.src[p][(int64_t)r * g.stride[p] + c];
}

__device__ __forceinline__ uint64_t enc_min64_wave(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
    const uint64_t o = (uint64_t)hi << 32 | lo;
    v = o < v ? o : v;
  }
  return v;
}

// ---- motion search ---------------------------------------------------------------------------------------------------------------
// the 16 x 16 source of the macro block at (x0, y0) into s_src (rows of four words), by threads 0..63
__device__ __forceinline__ void enc_me_load_src(uint32_t *s_src, const EncPlanes &g, int x0, int y0) {
  const int tid = (int)threadIdx.x;
  if (tid < 64) {
    const int r = tid >> 2, c = (tid & 3) * 4;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= (uint32_t)enc_src_px(g, 0, x0 + c + b, y0 + r) << (8 * b);
    s_src[tid] = v;
  }
}

// the intra SAD of luma block bq (0..3) of s_src against its rounded mean
__device__ __forceinline__ uint32_t enc_me_intra_sad(const uint32_t *s_src, int bq) {
  const int bx = (bq & 1) * 2, by = (bq >> 1) * 8;
  uint32_t sum = 0;
  for (int r = 0; r < 8; r++) sum = __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx + 1], 0u, __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx], 0u, sum));
  const uint32_t m = ((sum + 32) >> 6) * 0x01010101u;
  uint32_t v = 0;
  for (int r = 0; r < 8; r++) v = __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx + 1], m, __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx], m, v));
  return v;
}

// the full-pel vector of a search key (its low 16 bits: the candidate's raster index)
__device__ __forceinline__ void enc_me_key_vec(uint64_t best, int &bdx, int &bdy) {
  const int bci = (int)(best & 0xFFFF);
  bdx = bci % kMeSide - kMeRange;
  bdy = bci / kMeSide - kMeRange;
}

// the half-pel refinement's choice around the full-pel vector (bdx, bdy) of key `best`: the centre keeps its full-pel key with
// raster index 4 of the 3 x 3 neighbourhood; hp: the eight neighbours' SADs.  Returns the SAD of the vector chosen
__device__ __forceinline__ int enc_hp_choose(uint64_t best, int bdx, int bdy, const uint32_t *hp, int &mvx, int &mvy) {
  uint64_t cb = (best >> 16 << 16) | 4u;
  int bk = 4;
  for (int hk = 0; hk < 8; hk++) {
    const int k9 = hk < 4 ? hk : hk + 1;
    const int x = 2 * bdx + k9 % 3 - 1, y = 2 * bdy + k9 / 3 - 1;
    const uint64_t key = (uint64_t)hp[hk] << 32 | (uint64_t)(abs(x) + abs(y)) << 16 | (uint64_t)k9;
    if (key < cb) {
      cb = key;
      bk = k9;
    }
  }
  mvx = 2 * bdx + bk % 3 - 1;
  mvy = 2 * bdy + bk / 3 - 1;
  return (int)(cb >> 32);
}
__device__ __forceinline__ int enc_hp_choose(uint64_t best, const uint32_t *hp, int &mvx, int &mvy) {
  int bdx, bdy;
  enc_me_key_vec(best, bdx, bdy);
  return enc_hp_choose(best, bdx, bdy, hp, mvx, mvy);
}

struct EncMe {   // what the search finds: the SADs of vector 0, of the vector chosen and of INTRA, and the vector (half pixels)
  int s0, smv, si, mvx, mvy;
};

// The search of macro block blockIdx.x (raster, rows from the bottom) against R, by the whole work group of 256.  True in thread
// 0, which holds the result.
__device__ __forceinline__ bool enc_me_search(EncMe &out, const EncPlanes &g, const EncRef &R, int nmbx) {
  __shared__ uint32_t s_win[kMeWin * kMeWin / 4];
  __shared__ uint32_t s_src[16 * 4];
  __shared__ uint64_t s_best[4];
  __shared__ uint32_t s_hp[8], s_s0, s_si;
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int mb = (int)blockIdx.x, mbx = mb % nmbx, mby = mb / nmbx, x0 = mbx * 16, y0 = mby * 16;
  {
    const uint8_t *pl = R.plane[0];
    const int W = R.w[0], H = R.h[0];
    for (int i = tid; i < kMeWin * kMeWin / 4; i += 256) {
      const int r = i / (kMeWin / 4), c = (i - r * (kMeWin / 4)) * 4;
      const uint8_t *row = pl + (int64_t)min(max(y0 - 16 + r, 0), H - 1) * R.stride[0];
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) v |= (uint32_t)row[min(max(x0 - 16 + c + b, 0), W - 1)] << (8 * b);
      s_win[i] = v;
    }
  }
  enc_me_load_src(s_src, g, x0, y0);
  if (tid < 8) s_hp[tid] = 0;
  if (tid == 8) s_si = 0;
  __syncthreads();
  // full pel: key (SAD, |mvx| + |mvy|, raster index of the candidate), the least wins
  uint64_t best = ~0ull;
  for (int ci = tid; ci < kMeSide * kMeSide; ci += 256) {
    const int dy = ci / kMeSide - kMeRange, dx = ci % kMeSide - kMeRange;
    const int cc = dx + 16, q = cc >> 2, sh = cc & 3;
    uint32_t sad = 0;
#pragma unroll 4
    for (int r = 0; r < 16; r++) {
      const uint32_t *row = s_win + (r + dy + 16) * (kMeWin / 4) + q;
      uint32_t a[5];
#pragma unroll
      for (int k = 0; k < 5; k++) a[k] = row[k];
#pragma unroll
      for (int k = 0; k < 4; k++) sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a[k + 1], a[k], (uint32_t)sh), s_src[r * 4 + k], sad);
    }
    if (dx == 0 && dy == 0) s_s0 = sad;
    const uint64_t key = (uint64_t)sad << 32 | (uint64_t)(2 * (abs(dx) + abs(dy))) << 16 | (uint64_t)ci;
    best = key < best ? key : best;   // (no two keys are equal: each holds its candidate's index, so `<` and `<=` pick the same)
  }
  best = enc_min64_wave(best);
  if (lane == 0) s_best[w] = best;
  if (tid >= 64 && tid < 68) atomicAdd(&s_si, enc_me_intra_sad(s_src, tid - 64));   // the four luma blocks
  __syncthreads();
  best = s_best[0];
#pragma unroll
  for (int k = 1; k < 4; k++) best = s_best[k] < best ? s_best[k] : best;
  int bdx, bdy;
  enc_me_key_vec(best, bdx, bdy);
  // half pel: the eight neighbours of 2 (bdx, bdy); 16 lanes a candidate, one row each
  if (tid < 128) {
    const int hk = tid >> 4, k9 = hk < 4 ? hk : hk + 1, r = tid & 15;
    const int mvx = 2 * bdx + k9 % 3 - 1, mvy = 2 * bdy + k9 / 3 - 1;
    int mx, mx2, my, my2;
    mv_axis(mvx, false, mx, mx2);
    mv_axis(mvy, false, my, my2);
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s_win);
    const uint8_t *ra = win + (r + my + 16) * kMeWin + mx + 16, *rb = win + (r + my + my2 + 16) * kMeWin + mx + mx2 + 16;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(s_src) + r * 16;
    uint32_t sad = 0;
#pragma unroll
    for (int c = 0; c < 16; c++) sad += (uint32_t)abs((int)src[c] - (((int)ra[c] + (int)rb[c]) >> 1));
    atomicAdd(&s_hp[hk], sad);
  }
  __syncthreads();
  if (tid != 0) return false;
  out.smv = enc_hp_choose(best, bdx, bdy, s_hp, out.mvx, out.mvy);
  out.s0 = (int)s_s0;
  out.si = (int)s_si;
  return true;
}

// grid: one work group per macro block (raster, rows from the bottom).  lambda: the frame's inter luma step at zig-zag index 1.
__global__ __launch_bounds__(256) void k_enc_me(uint32_t *mb_out, EncPlanes g, EncRef R, int nmbx, int lambda) {
  EncMe m;
  if (!enc_me_search(m, g, R, nmbx)) return;
  int mode = m.smv + lambda < m.s0 ? kEncPixMv : kEncPixNomv;
  const int sinter = mode == kEncPixMv ? m.smv : m.s0;
  if (m.si + 4 * lambda < sinter) mode = kEncPixIntra;
  mb_out[blockIdx.x] = mode == kEncPixMv ? (uint32_t)mode | ((uint32_t)m.mvx & 0xFFu) << 8 | ((uint32_t)m.mvy & 0xFFu) << 16 : (uint32_t)mode;
}

// ---- block prediction ------------------------------------------------------------------------------------------------------------
// the macro block (raster) of fragment (p, fx, fy)
__device__ __forceinline__ int enc_mb_of(int p, int fx, int fy, int hdec, int vdec, int nmbx) {
  const int mbx = p ? fx >> (1 - hdec) : fx >> 1, mby = p ? fy >> (1 - vdec) : fy >> 1;
  return mby * nmbx + mbx;
}

__device__ __forceinline__ int enc_round_div(int v, int shift) {   // the decoder's round_div: ties away from zero
  const int half = 1 << (shift - 1);
  return v >= 0 ? (v + half) >> shift : -((-v + half) >> shift);
}

struct EncPred {   // how a block is predicted: the pixel mode, the vector of its plane, the reference's plane
  int pix, mvx, mvy;
  const uint8_t *pl;
};

// the prediction of block (p, fx, fy) from its macro block's word.  Word: uint32_t (k_enc_me's: mode | mvx << 8 | mvy << 16, PREV
// only; G is not read) or uint4 (k_enc_me_all's, thip_encode_modes.h: GOLD modes, and MV_FOUR with the block's own vector in luma
// and the vector the decoder derives in chroma -- thip_frontend.cpp, spec 7.5)
// (enc_word_pred: from the word itself -- k_enc_mb_rd of thip_encode_rd.h predicts from each candidate's word before one is written)
template <class Word>
__device__ __forceinline__ EncPred enc_word_pred(const Word &mw, const EncRef &R, const EncRef &G, int p, int fx, int fy) {
  if constexpr (sizeof(Word) == sizeof(uint32_t)) {
    return {(int)(mw & 0xFF), (int)(int8_t)(mw >> 8), (int)(int8_t)(mw >> 16), R.plane[p]};
  } else {
    const int pix = (int)(mw.x & 0xFF);
    int mvx = (int)(int8_t)(mw.x >> 8), mvy = (int)(int8_t)(mw.x >> 16);
    if (pix == kEncPixFour) {
      // the block vectors A, B (bottom), C, D (top)
      const int row = fy & 1;
      const uint32_t rw = row ? mw.z : mw.y;   // the two vectors of the block's row
      const int ax = (int)(int8_t)rw, ay = (int)(int8_t)(rw >> 8), bx = (int)(int8_t)(rw >> 16), by = (int)(int8_t)(rw >> 24);
      if (p == 0 || (!R.hdec && !R.vdec)) {
        mvx = fx & 1 ? bx : ax;
        mvy = fx & 1 ? by : ay;
      } else if (R.hdec && R.vdec) {
        const uint32_t o = row ? mw.y : mw.z;   // (the other row)
        mvx = enc_round_div(ax + bx + (int)(int8_t)o + (int)(int8_t)(o >> 16), 2);
        mvy = enc_round_div(ay + by + (int)(int8_t)(o >> 8) + (int)(int8_t)(o >> 24), 2);
      } else {   // 4:2:2: the row's two
        mvx = enc_round_div(ax + bx, 1);
        mvy = enc_round_div(ay + by, 1);
      }
    }
    const uint8_t *pr = R.plane[p], *pg = G.plane[p];   // (both loaded, then the value chosen: choosing the struct copied both to scratch)
    return {pix, mvx, mvy, enc_pix_gold(pix) ? pg : pr};
  }
}
template <class Word>
__device__ __forceinline__ EncPred enc_block_pred(const Word *mbw, int nmbx, const EncRef &R, const EncRef &G, int p, int fx, int fy) {
  return enc_word_pred(mbw[enc_mb_of(p, fx, fy, R.hdec, R.vdec, nmbx)], R, G, p, fx, fy);
}

// The predictor pixels of block (p, fx, fy) under `pr`, as EncSrcBlock holds the source's: the decoder's offsets (mv_axis, quarter
// pixels on a decimated chroma axis) and the clamped columns of its two reads, once for all the block's rows
struct EncPredBlock {
  bool intra;
  const uint8_t *pl;
  int stride, h1, ya, yb;   // row r reads plane rows ya + r and yb + r, clamped to [0, h1]
  int ca[8], cb[8];
};
__device__ __forceinline__ EncPredBlock enc_pred_block(const EncRef &R, const EncPred &pr, int p, int fx, int fy) {
  int mx, mx2, my, my2;
  mv_axis(pr.mvx, p != 0 && R.hdec, mx, mx2);
  mv_axis(pr.mvy, p != 0 && R.vdec, my, my2);
  EncPredBlock b;
  b.intra = pr.pix == kEncPixIntra;
  b.pl = pr.pl;
  b.stride = R.stride[p];
  b.h1 = R.h[p] - 1;
  b.ya = fy * 8 + my;
  b.yb = b.ya + my2;
  const int xa = fx * 8 + mx, xb = xa + mx2, w1 = R.w[p] - 1;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    b.ca[c] = min(max(xa + c, 0), w1);
    b.cb[c] = min(max(xb + c, 0), w1);
  }
  return b;
}

// row r of a block's residual: the source less its prediction (the decoder's truncating average of the two reads), 128 for an
// INTRA block (enc_stage_rows' row)
__device__ __forceinline__ void enc_residual_row(int v[8], const EncSrcBlock &s, const EncPredBlock &b, int r) {
  const uint8_t *row = enc_src_row(s, r);
  if (b.intra) {
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = (int)row[s.cx[c]] - 128;
  } else {
    const uint8_t *ra = b.pl + (int64_t)min(max(b.ya + r, 0), b.h1) * b.stride;
    const uint8_t *rb = b.pl + (int64_t)min(max(b.yb + r, 0), b.h1) * b.stride;
#pragma unroll
    for (int c = 0; c < 8; c++) v[c] = (int)row[s.cx[c]] - (((int)ra[b.ca[c]] + (int)rb[b.cb[c]]) >> 1);
  }
}

// The body of k_enc_inter_fq (two classes, k_enc_me's words) and k_enc_inter_fq_all (three, k_enc_me_all's).  levels [n][64], dcq
// [nfrags], cmap [nfrags], dclast [ceil(nfrags / 256)][kClasses] (zeroed before), overflow: zeroed for the tokens.  dequant:
// [2][3][64] zig-zag, the intra then the inter tables of the frame's qi
template <int kClasses, class Word>
__device__ __forceinline__ void enc_inter_fq(int16_t *levels, int16_t *dcq, uint8_t *cmap, uint32_t *dclast, uint32_t *overflow,
                                             const int32_t *coded_order, const EncPlanes &g, const EncRef &R, const EncRef &G,
                                             const Word *mbw, int nmbx, const uint16_t *dequant, int64_t n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;
  __shared__ __attribute__((aligned(16))) uint2 s_t[6 * 64];   // per (intra / inter, plane), by natural position
  enc_quant_tables(s_t, dequant, 6);
  __shared__ int4 s_x[4 * 128];
  int4 *lds = s_x + (threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t b0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2;
  const int64_t k = b0 + b;
  const int fi = coded_order[min(k, n - 1)];   // (a lane past the last block: any block's, it stores nothing)
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  const EncPred pr = enc_block_pred(mbw, nmbx, R, G, p, fx, fy);
  const EncSrcBlock sb = enc_src_block(g, p, fx, fy);
  const EncPredBlock pb = enc_pred_block(R, pr, p, fx, fy);
  enc_stage_rows(lds, b, j, k < n, [&](int r, int v[8]) { enc_residual_row(v, sb, pb, r); });
  __syncthreads();   // (the tables too)
  fdct_quantize4_lds(lds, s_t + 64 * ((pr.pix == kEncPixIntra ? 0 : 3) + p), b, j);
  enc_fq_tail<kClasses>(levels, dcq, cmap, dclast, lds, [=](int) { return lds; }, lds, b0, n, fi, pr.pix);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_enc_inter_fq(int16_t *levels, int16_t *dcq, uint8_t *cmap, uint32_t *dclast,
                                                      uint32_t *overflow, const int32_t *coded_order, EncPlanes g, EncRef R,
                                                      const uint32_t *mb_mode, int nmbx, const uint16_t *dequant, int64_t n) {
  enc_inter_fq<2>(levels, dcq, cmap, dclast, overflow, coded_order, g, R, R, mb_mode, nmbx, dequant, n);
}

// inclusive max-scan over the 256 threads of a work group (s_w: 4 words of LDS)
__device__ __forceinline__ uint32_t enc_block_max_scan(uint32_t v, uint32_t *s_w) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(v, d);
    if (lane >= d) v = max(v, y);
  }
  if (lane == 63) s_w[w] = v;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 3; q++) v = q < w ? max(v, s_w[q]) : v;
  __syncthreads();
  return v;
}

// The body of k_enc_inter_dc (two reference classes) and k_enc_inter_dc3 (three, thip_encode_modes.h).  grid: ceil(nfrags / 256)
// work groups over the RASTER fragment index.  dcr [nfrags]: the DC residual of every coded fragment; dclast [chunks][kClasses]
template <int kClasses>
__device__ __forceinline__ void enc_inter_dc(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast,
                                             const EncPlanes &g, int64_t nfrags) {
  __shared__ uint32_t s_w[4], s_pre[kClasses], s_own[kClasses][256];
  const int tid = (int)threadIdx.x;
  if (tid < kClasses) s_pre[tid] = 0;
  const int64_t fi64 = (int64_t)blockIdx.x * 256 + tid;
  const int fi = (int)fi64;
  const int cl = fi64 < nfrags ? (int)cmap[fi] : 0;
#pragma unroll
  for (int c = 0; c < kClasses; c++) s_own[c][tid] = cl == c + 1 ? (uint32_t)fi + 1u : 0u;
  __syncthreads();
  // the last coded fragment (+1) of each class in the earlier chunks ...
  uint32_t pm[kClasses] = {};
  for (int c = tid; c < (int)blockIdx.x; c += 256) {
#pragma unroll
    for (int q = 0; q < kClasses; q++) pm[q] = max(pm[q], dclast[kClasses * c + q]);
  }
#pragma unroll
  for (int q = 0; q < kClasses; q++)
    if (pm[q]) atomicMax(&s_pre[q], pm[q]);
  // ... and in this chunk before the thread's own: the inclusive max-scan of the values shifted by one
  uint32_t xl = 0;
#pragma unroll
  for (int q = 0; q < kClasses; q++) {
    const uint32_t x = enc_block_max_scan(tid ? s_own[q][tid - 1] : 0u, s_w);   // (its barriers also publish s_pre)
    if (cl == q + 1) xl = x;
  }
  if (!cl) return;
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  const int nh = g.nh[p];
  int l = 0, ul = 0, u = 0, ur = 0, msk = 0;
  if (fx > 0 && cmap[fi - 1] == cl) { l = dcq[fi - 1]; msk |= 1; }
  if (fy > 0) {
    if (fx > 0 && cmap[fi - nh - 1] == cl) { ul = dcq[fi - nh - 1]; msk |= 2; }
    if (cmap[fi - nh] == cl) { u = dcq[fi - nh]; msk |= 4; }
    if (fx + 1 < nh && cmap[fi - nh + 1] == cl) { ur = dcq[fi - nh + 1]; msk |= 8; }
  }
  int pred;
  if (msk) {
    pred = enc_dc_pred(msk, l, ul, u, ur);
  } else {
    const uint32_t last = max(xl, s_pre[cl - 1]);   // (0: none)
    pred = last > (uint32_t)g.froff[p] ? (int)dcq[last - 1] : 0;
  }
  dcr[fi] = (int16_t)((int)dcq[fi] - pred);
}

__global__ __launch_bounds__(256) void k_enc_inter_dc(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast,
                                                      EncPlanes g, int64_t nfrags) {
  enc_inter_dc<2>(dcr, dcq, cmap, dclast, g, nfrags);
}

// tok [n][kEncTokWords], mask [n], chunk_cnt [gridDim.x][3][64], overflow: as k_enc_intra_tok, over the coded blocks
__global__ __launch_bounds__(256) void k_enc_inter_tok(uint32_t *tok, uint64_t *mask, uint32_t *chunk_cnt, uint32_t *overflow,
                                                       const int16_t *levels, const int16_t *dcr, const uint8_t *cmap,
                                                       const int32_t *coded_order, EncPlanes g, int64_t n) {
  __shared__ uint32_t s_cnt[3 * 64];
  if (threadIdx.x < 192) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    const int fi = coded_order[k];
    if (cmap[fi]) {
      const int ovf = enc_block_tokens(tok + k * kEncTokWords, mask[k], s_cnt, levels + k * 64, (int)dcr[fi], enc_plane_of(g, fi));
      if (ovf) atomicAdd(overflow, (uint32_t)ovf);
    } else {
      mask[k] = 0;
    }
  }
  __syncthreads();
  if (threadIdx.x < 192) chunk_cnt[(int64_t)blockIdx.x * 192 + threadIdx.x] = s_cnt[threadIdx.x];
}

// ---- the launches, stated once: th_encode_* (thip_encode.hip) and thip_enc_inter_stage (theora_hip.h) both call these -----------
// Five modes here; the launches over k_enc_me_all's words are their overloads in thip_encode_modes.h, k_rate_me's and
// k_enc_mb_modes' are rate_launch_me (thip_rate.h) and cut_launch_mb_modes (thip_encode_cut.h).
struct InterBufs {        // device memory the transform-and-quantise launch writes
  int16_t *levels;        // [n][64], coded order
  int16_t *dcq;           // [n], raster
  uint8_t *cmap;          // [n], raster
  uint32_t *dclast;       // [ceil(n / 256)][classes], zeroed on the same stream before
  uint32_t *overflow;     // one word (zeroed by the launch, for the token kernel)
};

// the search and the decision: k_enc_me's word of each of the nmbs macro blocks into mb
inline hipError_t inter_launch_search(uint32_t *mb, const EncPlanes &g, const EncRef &R, int nmbx, int nmbs, int lambda, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_me, dim3((unsigned)nmbs), dim3(256), 0, stream, mb, g, R, nmbx, lambda);
  return hipGetLastError();
}

// transform and quantise over k_enc_me's words: order [n] (the coded order), dequant [2][3][64] (device, zig-zag)
inline hipError_t inter_launch_fq(const InterBufs &o, const int32_t *order, const EncPlanes &g, const EncRef &R, const uint32_t *mb,
                                  int nmbx, const uint16_t *dequant, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_inter_fq, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, stream, o.levels, o.dcq, o.cmap, o.dclast,
                     o.overflow, order, g, R, mb, nmbx, dequant, n);
  return hipGetLastError();
}

// the DC residuals with two classes: dclast [ceil(n / 256)][2] as inter_launch_fq left it
inline hipError_t inter_launch_dc(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast, const EncPlanes &g,
                                  int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_inter_dc, dim3((unsigned)((n + kEncChunk - 1) / kEncChunk)), dim3(256), 0, stream, dcr, dcq, cmap, dclast, g, n);
  return hipGetLastError();
}

// an inter frame's tokens (th_encode_* and thip_enc_tok_stage): the coded blocks' of levels [n][64] (coded order) with the DC residuals
// dcr [n] and the map cmap [n] (raster); an uncoded block gets mask 0 and nothing else
inline hipError_t tok_launch_inter(const TokBufs &o, const int16_t *levels, const int16_t *dcr, const uint8_t *cmap, const int32_t *order,
                                   const EncPlanes &g, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_inter_tok, dim3(enc_chunks(n)), dim3(256), 0, stream, o.tok, o.mask, o.chunk_cnt, o.overflow, levels, dcr,
                     cmap, order, g, n);
  return hipGetLastError();
}

}  // namespace thip
