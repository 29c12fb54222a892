// thip_encode_inter.h -- the device stage of an inter frame of th_encode_* (thip_encode.hip; the bitstream is stated in
// theoraenc_hip.h).  Everything is in bitstream coordinates: rows counted from the BOTTOM of the coded frame (spec 2.2), vectors
// in half pixels with y pointing up.  The reference is PREV, a frame of the encoder's own decoder: three planes, bitstream row order,
// no border (reads clamp their coordinates, as the decoder's motion-compensated reads do).
//
//   k_enc_me        one work group a macro block: the 48 x 48 reference window around it (the search range plus one pixel for
//                   the half-pel reads, coordinates clamped) and the 16 x 16 source go through LDS; a lane takes one full-pel
//                   candidate in four (961 of them: every (dx, dy) in [-15, 15]^2), a row costs four v_sad_u8 on alignbyte-shifted
//                   words.  The best full-pel vector is refined over its eight half-pel neighbours with the decoder's own
//                   prediction (mv_axis, a truncating average of two reads).  Out: one word a macro block (raster order, rows from
//                   the bottom): the pixel mode (NOMV / INTRA / MV) | mvx << 8 | mvy << 16 (bytes, zero unless MV).
//   k_enc_inter_fq  k_enc_intra_fq for an inter frame: the prediction (128 for INTRA, PREV through the macro block's vector, with
//                   the chroma vector of spec 7.9.4 for 4:2:0 and 4:2:2) is subtracted, the block is transformed and quantised
//                   with the intra or inter table of its plane, and its coded flag is set: always for INTRA and MV macro blocks,
//                   for NOMV ones when a level is not zero.  cmap[fi] (raster): 0 uncoded, 1 coded intra, 2 coded from PREV.  For
//                   the DC predictor it records, per 256 raster fragments and class, the last coded fragment (+1, atomicMax).
//   k_enc_inter_dc  the DC residuals of spec 7.8 with reference classes: a neighbour counts when it is coded and of the same
//                   class; a block with none predicts from the last coded DC of its class before it in the plane's raster order --
//                   a segmented "last value" scan (a max-scan of fragment indices, cut at the plane's first fragment).
//   k_enc_inter_tok k_enc_intra_tok over the coded blocks only (an uncoded block has no tokens and an empty mask), with the DC
//                   residual of k_enc_inter_dc.  k_enc_intra_scan and k_enc_intra_scatter then serve both frame types.
#pragma once
#include "thip_encode.h"

namespace thip {

constexpr int kMeRange = 15;              // full-pel search: dx, dy in [-15, 15]
constexpr int kMeSide = 31;               // candidates a side
constexpr int kMeWin = 48;                // window side: 16 + 2 * (15 + 1)
enum { kEncPixNomv = 0, kEncPixIntra = 1, kEncPixMv = 2 };

struct EncRef {            // PREV, bitstream row order
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

// the predictor pixel at (x, y) of plane p for vector (mvx, mvy) (half pixels of luma): the decoder's offsets (mv_axis, quarter
// pixels on a decimated chroma axis) and its truncating average of the two reads, coordinates clamped
__device__ __forceinline__ int enc_pred_px(const EncRef &R, int p, int x, int y, int mvx, int mvy) {
  int mx, mx2, my, my2;
  mv_axis(mvx, p != 0 && R.hdec, mx, mx2);
  mv_axis(mvy, p != 0 && R.vdec, my, my2);
  const uint8_t *pl = R.plane[p];
  const int W = R.w[p], H = R.h[p];
  const int a = pl[(int64_t)min(max(y + my, 0), H - 1) * R.stride[p] + min(max(x + mx, 0), W - 1)];
  const int b = pl[(int64_t)min(max(y + my + my2, 0), H - 1) * R.stride[p] + min(max(x + mx + mx2, 0), W - 1)];
  return (a + b) >> 1;
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

// grid: one work group per macro block (raster, rows from the bottom).  lambda: the frame's inter luma step at zig-zag index 1.
// k_rate_me (thip_rate.h) copies the search and writes its statistics instead of the decision: a fix here belongs there too.
__global__ __launch_bounds__(256) void k_enc_me(uint32_t *mb_out, EncPlanes g, EncRef R, int nmbx, int lambda) {
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
  if (tid < 64) {
    const int r = tid >> 2, c = (tid & 3) * 4;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) v |= (uint32_t)enc_src_px(g, 0, x0 + c + b, y0 + r) << (8 * b);
    s_src[tid] = v;
  }
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
    best = key < best ? key : best;
  }
  best = enc_min64_wave(best);
  if (lane == 0) s_best[w] = best;
  if (tid >= 64 && tid < 68) {   // intra SAD of the four luma blocks against their rounded means
    const int bq = tid - 64, bx = (bq & 1) * 2, by = (bq >> 1) * 8;
    uint32_t sum = 0;
    for (int r = 0; r < 8; r++) sum = __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx + 1], 0u, __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx], 0u, sum));
    const uint32_t m = ((sum + 32) >> 6) * 0x01010101u;
    uint32_t v = 0;
    for (int r = 0; r < 8; r++) v = __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx + 1], m, __builtin_amdgcn_sad_u8(s_src[(by + r) * 4 + bx], m, v));
    atomicAdd(&s_si, v);
  }
  __syncthreads();
  best = s_best[0];
#pragma unroll
  for (int k = 1; k < 4; k++) best = s_best[k] < best ? s_best[k] : best;
  const int bci = (int)(best & 0xFFFF);
  const int bdx = bci % kMeSide - kMeRange, bdy = bci / kMeSide - kMeRange;
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
  if (tid == 0) {
    uint64_t cb = (best >> 16 << 16) | 4u;   // the centre keeps its full-pel key, with raster index 4 of the 3 x 3 neighbourhood
    int bk = 4;
    for (int hk = 0; hk < 8; hk++) {
      const int k9 = hk < 4 ? hk : hk + 1;
      const int mvx = 2 * bdx + k9 % 3 - 1, mvy = 2 * bdy + k9 / 3 - 1;
      const uint64_t key = (uint64_t)s_hp[hk] << 32 | (uint64_t)(abs(mvx) + abs(mvy)) << 16 | (uint64_t)k9;
      if (key < cb) {
        cb = key;
        bk = k9;
      }
    }
    const int mvx = 2 * bdx + bk % 3 - 1, mvy = 2 * bdy + bk / 3 - 1;
    const int smv = (int)(cb >> 32), s0 = (int)s_s0, si = (int)s_si;
    int mode = smv + lambda < s0 ? kEncPixMv : kEncPixNomv;
    const int sinter = mode == kEncPixMv ? smv : s0;
    if (si + 4 * lambda < sinter) mode = kEncPixIntra;
    mb_out[mb] = mode == kEncPixMv ? (uint32_t)mode | ((uint32_t)mvx & 0xFFu) << 8 | ((uint32_t)mvy & 0xFFu) << 16 : (uint32_t)mode;
  }
}

// levels [n][64], dcq [nfrags], cmap [nfrags], dclast [ceil(nfrags / 256)][2] (zeroed before), overflow: zeroed for the tokens.
// dequant: [2][3][64] zig-zag, the intra then the inter tables of the frame's qi
__global__ __launch_bounds__(256) void k_enc_inter_fq(int16_t *levels, int16_t *dcq, uint8_t *cmap, uint32_t *dclast,
                                                      uint32_t *overflow, const int32_t *coded_order, EncPlanes g, EncRef R,
                                                      const uint32_t *mb_mode, int nmbx, const uint16_t *dequant, int64_t n) {
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
    const uint32_t mw = mb_mode[mby * nmbx + mbx];
    pix = (int)(mw & 0xFF);
    const int mvx = (int)(int8_t)(mw >> 8), mvy = (int)(int8_t)(mw >> 16);
    tab = (pix == kEncPixIntra ? 0 : 3) + p;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int r = 2 * j + h, y = fy * 8 + r;
      int v[8];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const int x = fx * 8 + c;
        v[c] = enc_src_px(g, p, x, y) - (pix == kEncPixIntra ? 128 : enc_pred_px(R, p, x, y, mvx, mvy));
      }
      lds[b * 8 + ((r + b) & 7)] = make_int4((v[0] & 0xFFFF) | (v[1] << 16), (v[2] & 0xFFFF) | (v[3] << 16),
                                             (v[4] & 0xFFFF) | (v[5] << 16), (v[6] & 0xFFFF) | (v[7] << 16));
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
  // any level of the block not zero: lane j looks at rows 2j, 2j + 1 of its (rotated) zig-zag pieces
  const int4 r0 = lds[b * 8 + ((2 * j + b) & 7)], r1 = lds[b * 8 + ((2 * j + 1 + b) & 7)];
  int nz = (r0.x | r0.y | r0.z | r0.w | r1.x | r1.y | r1.z | r1.w) != 0;
  nz |= __shfl_xor(nz, 1);
  nz |= __shfl_xor(nz, 2);
  if (j == 0 && k < n) {
    dcq[fi] = (int16_t)lds[b * 8 + (b & 7)].x;
    const int cls = pix == kEncPixIntra ? 1 : 2;
    const bool coded = pix != kEncPixNomv || nz;
    cmap[fi] = coded ? (uint8_t)cls : (uint8_t)0;
    if (coded) atomicMax(&dclast[(fi >> 8) * 2 + cls - 1], (uint32_t)fi + 1u);
  }
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

// grid: ceil(nfrags / 256) work groups over the RASTER fragment index.  dcr [nfrags]: the DC residual of every coded fragment
__global__ __launch_bounds__(256) void k_enc_inter_dc(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast,
                                                      EncPlanes g, int64_t nfrags) {
  __shared__ uint32_t s_w[4], s_pre[2], s_own[2][256];
  const int tid = (int)threadIdx.x;
  if (tid < 2) s_pre[tid] = 0;
  const int64_t fi64 = (int64_t)blockIdx.x * 256 + tid;
  const int fi = (int)fi64;
  const int cl = fi64 < nfrags ? (int)cmap[fi] : 0;
  s_own[0][tid] = cl == 1 ? (uint32_t)fi + 1u : 0u;
  s_own[1][tid] = cl == 2 ? (uint32_t)fi + 1u : 0u;
  __syncthreads();
  // the last coded fragment (+1) of each class in the earlier chunks ...
  uint32_t pm0 = 0, pm1 = 0;
  for (int c = tid; c < (int)blockIdx.x; c += 256) {
    pm0 = max(pm0, dclast[2 * c]);
    pm1 = max(pm1, dclast[2 * c + 1]);
  }
  if (pm0) atomicMax(&s_pre[0], pm0);
  if (pm1) atomicMax(&s_pre[1], pm1);
  // ... and in this chunk before the thread's own: the inclusive max-scan of the values shifted by one
  const uint32_t x0 = enc_block_max_scan(tid ? s_own[0][tid - 1] : 0u, s_w);   // (its barriers also publish s_pre)
  const uint32_t x1 = enc_block_max_scan(tid ? s_own[1][tid - 1] : 0u, s_w);
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
    const uint32_t last = max(cl == 1 ? x0 : x1, s_pre[cl - 1]);   // (0: none)
    pred = last > (uint32_t)g.froff[p] ? (int)dcq[last - 1] : 0;
  }
  dcr[fi] = (int16_t)((int)dcq[fi] - pred);
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

}  // namespace thip
