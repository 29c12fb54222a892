// thip_encode_modes.h -- the device stage of an inter frame with all eight macro-block modes (TH_ENCCTL_THIP_SET_INTER_MODES;
// the bitstream is stated in theoraenc_hip.h, "All eight modes").  Coordinates, vectors and references as thip_encode_inter.h;
// the second reference is GOLD, the decoder's picture of the last key frame.
//
//   k_enc_me_all     k_enc_me with two references: both 48 x 48 windows (PREV, GOLD) and the source go through LDS.  A lane takes
//                    one full-pel candidate in four; for PREV it keeps the four 8 x 8 SADs in their own accumulators (the same
//                    v_sad_u8 count; their sum is the 16 x 16 SAD, so the macro-block search is k_enc_me's), and the least keys of the
//                    macro block and of each luma block; for GOLD the macro block's only.  Then 8 + 8 + 32 half-pel candidates
//                    (PREV and GOLD macro block, four blocks).  Out: one uint4 a macro block: x the pixel mode | vector << 8 (the
//                    vector of MV or GOLDEN_MV, else 0), y, z the block vectors 0, 1 and 2, 3 of MV_FOUR (16 bits each, else 0),
//                    w the GOLD search's vector.
//   k_enc_inter_fq_all  k_enc_inter_fq reading those words: the prediction is from PREV or GOLD, through the block's own vector in
//                    MV_FOUR luma and the vector the decoder derives for its chroma; cmap 1 intra, 2 PREV, 3 GOLD.
//   k_enc_inter_dc3  k_enc_inter_dc with the three reference classes.
// k_enc_inter_tok, k_enc_intra_scan and k_enc_intra_scatter only test cmap != 0 and serve this stage unchanged.
#pragma once
#include "thip_encode_inter.h"

namespace thip {

enum { kEncPixGoldNomv = 5, kEncPixGoldMv = 6, kEncPixFour = 7 };   // (the spec's mode numbers; 0..2 as thip_encode_inter.h)

__device__ __forceinline__ uint32_t enc_mv_pack(int x, int y) { return ((uint32_t)x & 0xFFu) | ((uint32_t)y & 0xFFu) << 8; }

// the half-pel refinement's choice (k_enc_me's): the centre keeps its full-pel key with index 4; hp: the eight neighbours' SADs
__device__ __forceinline__ int enc_hp_choose(uint64_t best, const uint32_t *hp, int &mvx, int &mvy) {
  const int bci = (int)(best & 0xFFFF);
  const int bdx = bci % kMeSide - kMeRange, bdy = bci / kMeSide - kMeRange;
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

// the SAD of one row of `n` pixels of the source (LDS, rows of 16) against the half-pel prediction of vector (mvx, mvy) from a
// window (LDS, rows of kMeWin, origin 16 pixels before the macro block's); (x, r) the row's first pixel in the macro block
__device__ __forceinline__ uint32_t enc_hp_row_sad(const uint32_t *win32, const uint32_t *src32, int x, int r, int n, int mvx, int mvy) {
  int mx, mx2, my, my2;
  mv_axis(mvx, false, mx, mx2);
  mv_axis(mvy, false, my, my2);
  const uint8_t *win = reinterpret_cast<const uint8_t *>(win32);
  const uint8_t *ra = win + (r + my + 16) * kMeWin + x + mx + 16, *rb = win + (r + my + my2 + 16) * kMeWin + x + mx + mx2 + 16;
  const uint8_t *src = reinterpret_cast<const uint8_t *>(src32) + r * 16 + x;
  uint32_t sad = 0;
  for (int c = 0; c < n; c++) sad += (uint32_t)abs((int)src[c] - (((int)ra[c] + (int)rb[c]) >> 1));
  return sad;
}

// grid: one work group per macro block (raster, rows from the bottom).  lambda: the frame's inter luma step at zig-zag index 1.
__global__ __launch_bounds__(256) void k_enc_me_all(uint4 *mb_out, EncPlanes g, EncRef R, EncRef G, int nmbx, int lambda) {
  __shared__ uint32_t s_win[kMeWin * kMeWin / 4], s_gwin[kMeWin * kMeWin / 4];
  __shared__ uint32_t s_src[16 * 4];
  __shared__ uint64_t s_best[6][4];   // PREV macro block, PREV blocks 0..3, GOLD macro block; per wave
  __shared__ uint32_t s_hp[48], s_s0, s_g0, s_si;
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int mb = (int)blockIdx.x, mbx = mb % nmbx, mby = mb / nmbx, x0 = mbx * 16, y0 = mby * 16;
  for (int i = tid; i < kMeWin * kMeWin / 4; i += 256) {
    const int r = i / (kMeWin / 4), c = (i - r * (kMeWin / 4)) * 4;
    const int64_t ro = (int64_t)min(max(y0 - 16 + r, 0), R.h[0] - 1) * R.stride[0];
    const uint8_t *row = R.plane[0] + ro, *grow = G.plane[0] + ro;   // (PREV and GOLD share the decoder's geometry)
    uint32_t v = 0, gv = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int x = min(max(x0 - 16 + c + b, 0), R.w[0] - 1);
      v |= (uint32_t)row[x] << (8 * b);
      gv |= (uint32_t)grow[x] << (8 * b);
    }
    s_win[i] = v;
    s_gwin[i] = gv;
  }
  if (tid < 64) {
    const int r = tid >> 2, c = (tid & 3) * 4;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= (uint32_t)enc_src_px(g, 0, x0 + c + b, y0 + r) << (8 * b);
    s_src[tid] = v;
  }
  if (tid < 48) s_hp[tid] = 0;
  if (tid == 48) s_si = 0;
  __syncthreads();
  // full pel: keys (SAD, 2 (|dx| + |dy|), raster index of the candidate), the least wins
  uint64_t best = ~0ull, gbest = ~0ull, bbest[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  for (int ci = tid; ci < kMeSide * kMeSide; ci += 256) {
    const int dy = ci / kMeSide - kMeRange, dx = ci % kMeSide - kMeRange;
    const int cc = dx + 16, q = cc >> 2, sh = cc & 3;
    uint32_t sb[4] = {0, 0, 0, 0}, sg = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {   // block rows: h = 0 blocks 0, 1 (the bottom ones), h = 1 blocks 2, 3
#pragma unroll 2
      for (int r8 = 0; r8 < 8; r8++) {
        const int r = 8 * h + r8;
        const uint32_t *row = s_win + (r + dy + 16) * (kMeWin / 4) + q, *grow = s_gwin + (r + dy + 16) * (kMeWin / 4) + q;
        uint32_t a[5], ga[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
          a[k] = row[k];
          ga[k] = grow[k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t sw = s_src[r * 4 + k];
          sb[2 * h + (k >> 1)] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a[k + 1], a[k], (uint32_t)sh), sw, sb[2 * h + (k >> 1)]);
          sg = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(ga[k + 1], ga[k], (uint32_t)sh), sw, sg);
        }
      }
    }
    const uint32_t sad = sb[0] + sb[1] + sb[2] + sb[3];
    if (dx == 0 && dy == 0) {
      s_s0 = sad;
      s_g0 = sg;
    }
    const uint64_t tail = (uint64_t)(2 * (abs(dx) + abs(dy))) << 16 | (uint64_t)ci;
    const uint64_t key = (uint64_t)sad << 32 | tail, gkey = (uint64_t)sg << 32 | tail;
    best = key < best ? key : best;
    gbest = gkey < gbest ? gkey : gbest;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const uint64_t bk = (uint64_t)sb[b] << 32 | tail;
      bbest[b] = bk < bbest[b] ? bk : bbest[b];
    }
  }
  best = enc_min64_wave(best);
  gbest = enc_min64_wave(gbest);
#pragma unroll
  for (int b = 0; b < 4; b++) bbest[b] = enc_min64_wave(bbest[b]);
  if (lane == 0) {
    s_best[0][w] = best;
#pragma unroll
    for (int b = 0; b < 4; b++) s_best[1 + b][w] = bbest[b];
    s_best[5][w] = gbest;
  }
  if (tid >= 64 && tid < 68) {   // intra SAD of the four luma blocks against their rounded means (k_enc_me's)
    const int bq = tid - 64, bx = (bq & 1) * 2, by = (bq >> 1) * 8;
    uint32_t sum = 0;
    for (int r = 0; r < 8; r++) sum = __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx + 1], 0u, __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx], 0u, sum));
    const uint32_t m = ((sum + 32) >> 6) * 0x01010101u;
    uint32_t v = 0;
    for (int r = 0; r < 8; r++) v = __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx + 1], m, __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx], m, v));
    atomicAdd(&s_si, v);
  }
  __syncthreads();
  // half pel.  Pass 1: the eight neighbours of the PREV (lanes 0..127) and GOLD (128..255) macro-block vectors, 16 lanes a
  // candidate, one row each.  Pass 2: the eight neighbours of each block's vector, 8 lanes a candidate, one row each.
  {
    const int gsel = tid >> 7, hk = (tid >> 4) & 7, k9 = hk < 4 ? hk : hk + 1, r = tid & 15;
    uint64_t k = s_best[gsel ? 5 : 0][0];
#pragma unroll
    for (int v = 1; v < 4; v++) k = s_best[gsel ? 5 : 0][v] < k ? s_best[gsel ? 5 : 0][v] : k;
    const int bci = (int)(k & 0xFFFF);
    const int mvx = 2 * (bci % kMeSide - kMeRange) + k9 % 3 - 1, mvy = 2 * (bci / kMeSide - kMeRange) + k9 / 3 - 1;
    atomicAdd(&s_hp[8 * gsel + hk], enc_hp_row_sad(gsel ? s_gwin : s_win, s_src, 0, r, 16, mvx, mvy));
  }
  {
    const int b = tid >> 6, hk = (tid >> 3) & 7, k9 = hk < 4 ? hk : hk + 1, r = tid & 7;
    uint64_t k = s_best[1 + b][0];
#pragma unroll
    for (int v = 1; v < 4; v++) k = s_best[1 + b][v] < k ? s_best[1 + b][v] : k;
    const int bci = (int)(k & 0xFFFF);
    const int mvx = 2 * (bci % kMeSide - kMeRange) + k9 % 3 - 1, mvy = 2 * (bci / kMeSide - kMeRange) + k9 / 3 - 1;
    atomicAdd(&s_hp[16 + 8 * b + hk], enc_hp_row_sad(s_win, s_src, (b & 1) * 8, (b >> 1) * 8 + r, 8, mvx, mvy));
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t kb[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      kb[c] = s_best[c][0];
#pragma unroll
      for (int v = 1; v < 4; v++) kb[c] = s_best[c][v] < kb[c] ? s_best[c][v] : kb[c];
    }
    int mvx, mvy, gx, gy, bx[4], by[4];
    const int smv = enc_hp_choose(kb[0], s_hp, mvx, mvy);
    const int gmv = enc_hp_choose(kb[5], s_hp + 8, gx, gy);
    int s4 = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) s4 += enc_hp_choose(kb[1 + b], s_hp + 16 + 8 * b, bx[b], by[b]);
    const int s0 = (int)s_s0, g0 = (int)s_g0, si = (int)s_si;
    // the mode rule of theoraenc_hip.h: PREV with one vector, four vectors, GOLD, INTRA; ties keep the earlier choice
    int mode = kEncPixNomv, C = s0, S = s0;
    if (smv + lambda < s0) {
      mode = kEncPixMv;
      C = smv + lambda;
      S = smv;
    }
    if (s4 + 4 * lambda < C) {
      mode = kEncPixFour;
      C = s4 + 4 * lambda;
      S = s4;
    }
    int gm = kEncPixGoldNomv, CG = g0 + lambda, SG = g0;
    if (gmv + 2 * lambda < g0 + lambda) {
      gm = kEncPixGoldMv;
      CG = gmv + 2 * lambda;
      SG = gmv;
    }
    if (CG < C) {
      mode = gm;
      S = SG;
    }
    if (si + 4 * lambda < S) mode = kEncPixIntra;
    const uint32_t v = mode == kEncPixMv ? enc_mv_pack(mvx, mvy) : mode == kEncPixGoldMv ? enc_mv_pack(gx, gy) : 0u;
    const bool four = mode == kEncPixFour;
    mb_out[mb] = make_uint4((uint32_t)mode | v << 8, four ? enc_mv_pack(bx[0], by[0]) | enc_mv_pack(bx[1], by[1]) << 16 : 0u,
                            four ? enc_mv_pack(bx[2], by[2]) | enc_mv_pack(bx[3], by[3]) << 16 : 0u, enc_mv_pack(gx, gy));
  }
}

__device__ __forceinline__ int enc_round_div(int v, int shift) {   // the decoder's round_div: ties away from zero
  const int half = 1 << (shift - 1);
  return v >= 0 ? (v + half) >> shift : -((-v + half) >> shift);
}

// enc_pred_px from the plane `pl` of R's geometry
__device__ __forceinline__ int enc_pred_px_pl(const EncRef &R, const uint8_t *pl, int p, int x, int y, int mvx, int mvy) {
  int mx, mx2, my, my2;
  mv_axis(mvx, p != 0 && R.hdec, mx, mx2);
  mv_axis(mvy, p != 0 && R.vdec, my, my2);
  const int W = R.w[p], H = R.h[p];
  const int a = pl[(int64_t)min(max(y + my, 0), H - 1) * R.stride[p] + min(max(x + mx, 0), W - 1)];
  const int b = pl[(int64_t)min(max(y + my + my2, 0), H - 1) * R.stride[p] + min(max(x + mx + mx2, 0), W - 1)];
  return (a + b) >> 1;
}

// as k_enc_inter_fq; mb_word: k_enc_me_all's words, G: GOLD (R's geometry), dclast [ceil(nfrags / 256)][3] (zeroed before)
__global__ __launch_bounds__(256) void k_enc_inter_fq_all(int16_t *levels, int16_t *dcq, uint8_t *cmap, uint32_t *dclast,
                                                          uint32_t *overflow, const int32_t *coded_order, EncPlanes g, EncRef R,
                                                          EncRef G, const uint4 *mb_word, int nmbx, const uint16_t *dequant,
                                                          int64_t n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;
  __shared__ __attribute__((aligned(16))) uint2 s_t[6 * 64];   // per (intra / inter, plane), by natural position
  for (int i = (int)threadIdx.x; i < 6 * 64; i += 256) {
    const int t = i >> 6, z = i & 63, pos = kFZigZag[z];
    const uint32_t dq = dequant[t * 64 + z];
    const uint32_t d = dq << 1;   // as k_enc_intra_fq
    const int l = 31 - __builtin_clz(d);
    const uint32_t tt = 1u + ((1u << (16 + l)) / d);
    const int m = (int)(int16_t)(tt - 0x10000u);
    s_t[t * 64 + pos] = make_uint2(dq | (uint32_t)(uint16_t)m << 16, (uint32_t)(l & 0xFF) | (uint32_t)z << 8);
  }
  __shared__ int4 s_x[4 * 128];
  int4 *lds = s_x + (threadIdx.x >> 6) * 128;
  const int lane = (int)threadIdx.x & 63, b = lane >> 2, j = lane & 3;
  const int64_t b0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> 2;
  const int64_t k = b0 + b;
  int p = 0, fi = 0, tab = 0, pix = kEncPixIntra;
  if (k < n) {
    fi = coded_order[k];
    p = enc_plane_of(g, fi);
    const int loc = fi - g.froff[p], fy = loc / g.nh[p], fx = loc - fy * g.nh[p];
    const int mbx = p ? fx >> (1 - R.hdec) : fx >> 1, mby = p ? fy >> (1 - R.vdec) : fy >> 1;
    const uint4 mw = mb_word[mby * nmbx + mbx];
    pix = (int)(mw.x & 0xFF);
    int mvx = (int)(int8_t)(mw.x >> 8), mvy = (int)(int8_t)(mw.x >> 16);
    if (pix == kEncPixFour) {
      // the block vectors A, B (bottom), C, D (top); chroma: the decoder's derivation (thip_frontend.cpp, 7.5)
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
    const bool gold = pix == kEncPixGoldNomv || pix == kEncPixGoldMv;
    const uint8_t *pl = gold ? G.plane[p] : R.plane[p];
    tab = (pix == kEncPixIntra ? 0 : 3) + p;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = 2 * j + h, y = fy * 8 + r;
      int vv[8];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const int x = fx * 8 + c;
        vv[c] = enc_src_px(g, p, x, y) - (pix == kEncPixIntra ? 128 : enc_pred_px_pl(R, pl, p, x, y, mvx, mvy));
      }
      lds[b * 8 + ((r + b) & 7)] = make_int4((vv[0] & 0xFFFF) | (vv[1] << 16), (vv[2] & 0xFFFF) | (vv[3] << 16),
                                             (vv[4] & 0xFFFF) | (vv[5] << 16), (vv[6] & 0xFFFF) | (vv[7] << 16));
    }
  } else {
    lds[b * 8 + ((2 * j + b) & 7)] = make_int4(0, 0, 0, 0);
    lds[b * 8 + ((2 * j + 1 + b) & 7)] = make_int4(0, 0, 0, 0);
  }
  __syncthreads();   // (the tables too)
  fdct_quantize4_lds(lds, s_t + 64 * tab, b, j);
  int4 *o = reinterpret_cast<int4 *>(levels) + b0 * 8;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int idx = q * 64 + lane, bb = idx >> 3, pc = idx & 7;
    if (b0 + bb < n) o[idx] = lds[bb * 8 + ((pc + bb) & 7)];
  }
  const int4 r0 = lds[b * 8 + ((2 * j + b) & 7)], r1 = lds[b * 8 + ((2 * j + 1 + b) & 7)];
  int nz = (r0.x | r0.y | r0.z | r0.w | r1.x | r1.y | r1.z | r1.w) != 0;
  nz |= __shfl_xor(nz, 1);
  nz |= __shfl_xor(nz, 2);
  if (j == 0 && k < n) {
    dcq[fi] = (int16_t)lds[b * 8 + (b & 7)].x;
    const int cls = pix == kEncPixIntra ? 1 : (pix == kEncPixGoldNomv || pix == kEncPixGoldMv) ? 3 : 2;
    const bool coded = pix != kEncPixNomv || nz;
    cmap[fi] = coded ? (uint8_t)cls : (uint8_t)0;
    if (coded) atomicMax(&dclast[(fi >> 8) * 3 + cls - 1], (uint32_t)fi + 1u);
  }
}

// k_enc_inter_dc with three reference classes (dclast [chunks][3])
__global__ __launch_bounds__(256) void k_enc_inter_dc3(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast,
                                                       EncPlanes g, int64_t nfrags) {
  __shared__ uint32_t s_w[4], s_pre[3], s_own[3][256];
  const int tid = (int)threadIdx.x;
  if (tid < 3) s_pre[tid] = 0;
  const int64_t fi64 = (int64_t)blockIdx.x * 256 + tid;
  const int fi = (int)fi64;
  const int cl = fi64 < nfrags ? (int)cmap[fi] : 0;
#pragma unroll
  for (int c = 0; c < 3; c++) s_own[c][tid] = cl == c + 1 ? (uint32_t)fi + 1u : 0u;
  __syncthreads();
  // the last coded fragment (+1) of each class in the earlier chunks ...
  uint32_t pm[3] = {0, 0, 0};
  for (int c = tid; c < (int)blockIdx.x; c += 256) {
#pragma unroll
    for (int q = 0; q < 3; q++) pm[q] = max(pm[q], dclast[3 * c + q]);
  }
#pragma unroll
  for (int q = 0; q < 3; q++)
    if (pm[q]) atomicMax(&s_pre[q], pm[q]);
  // ... and in this chunk before the thread's own: the inclusive max-scan of the values shifted by one
  uint32_t x[3];
#pragma unroll
  for (int q = 0; q < 3; q++) x[q] = enc_block_max_scan(tid ? s_own[q][tid - 1] : 0u, s_w);   // (its barriers publish s_pre)
  if (!cl) return;
  const int p = enc_plane_of(g, fi), nh = g.nh[p];
  const int loc = fi - g.froff[p], fy = loc / nh, fx = loc - fy * nh;
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
    const uint32_t xl = cl == 1 ? x[0] : cl == 2 ? x[1] : x[2];
    const uint32_t last = max(xl, s_pre[cl - 1]);   // (0: none)
    pred = last > (uint32_t)g.froff[p] ? (int)dcq[last - 1] : 0;
  }
  dcr[fi] = (int16_t)((int)dcq[fi] - pred);
}

}  // namespace thip
