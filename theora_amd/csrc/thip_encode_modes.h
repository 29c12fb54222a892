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
//   k_enc_me_cand    the same search (one body, enc_me_all) without the decision: every candidate's vector and SAD, for the
//                    rate-distortion mode decision of thip_encode_rd.h.
//   k_enc_inter_fq_all  enc_inter_fq (thip_encode_inter.h) over those words: the prediction is from PREV or GOLD, through the
//                    block's own vector in MV_FOUR luma and the vector the decoder derives for its chroma (enc_block_pred);
//                    cmap 1 intra, 2 PREV, 3 GOLD.
//   k_enc_inter_dc3  enc_inter_dc<3>: k_enc_inter_dc with the three reference classes.
// The source load, the SAD against the block means and the half-pel choice are enc_me_search's own pieces (enc_me_load_src,
// enc_me_intra_sad, enc_hp_choose); the windows and the full-pel loop carry two references and five keys here and stay apart.
// k_enc_inter_tok, k_enc_intra_scan and k_enc_intra_scatter only test cmap != 0 and serve this stage unchanged.
#pragma once
#include "thip_encode_inter.h"

namespace thip {

__device__ __forceinline__ uint32_t enc_mv_pack(int x, int y) { return ((uint32_t)x & 0xFFu) | ((uint32_t)y & 0xFFu) << 8; }

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

// The body of k_enc_me_all and, with kCand, of k_enc_me_cand: the same search without the decision, which thip_encode_rd.h's
// k_enc_mb_rd makes from real costs.  kCand writes two uint4 a macro block: x = pack(mvx, mvy) | pack(gx, gy) << 16, y = block
// vectors 0, 1, z = block vectors 2, 3, w = S0 | Smv << 16; then x = S4 | SI << 16, y = G0 | Gmv << 16, z = w = 0 (a SAD is at most
// 65 280).  lambda is not read then.
template <bool kCand>
__device__ __forceinline__ void enc_me_all(uint4 *mb_out, const EncPlanes &g, const EncRef &R, const EncRef &G, int nmbx, int lambda) {
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
  enc_me_load_src(s_src, g, x0, y0);
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
  if (tid >= 64 && tid < 68) atomicAdd(&s_si, enc_me_intra_sad(s_src, tid - 64));   // the four luma blocks
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
    if constexpr (kCand) {
      mb_out[2 * (int64_t)mb] = make_uint4(enc_mv_pack(mvx, mvy) | enc_mv_pack(gx, gy) << 16, enc_mv_pack(bx[0], by[0]) | enc_mv_pack(bx[1], by[1]) << 16,
                                            enc_mv_pack(bx[2], by[2]) | enc_mv_pack(bx[3], by[3]) << 16, (uint32_t)s0 | (uint32_t)smv << 16);
      mb_out[2 * (int64_t)mb + 1] = make_uint4((uint32_t)s4 | (uint32_t)si << 16, (uint32_t)g0 | (uint32_t)gmv << 16, 0u, 0u);
      return;
    }
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

// grid: one work group per macro block (raster, rows from the bottom).  lambda: the frame's inter luma step at zig-zag index 1.
__global__ __launch_bounds__(256) void k_enc_me_all(uint4 *mb_out, EncPlanes g, EncRef R, EncRef G, int nmbx, int lambda) {
  enc_me_all<false>(mb_out, g, R, G, nmbx, lambda);
}

// the candidate form: cand [nmbs][2] (enc_me_all<true>)
__global__ __launch_bounds__(256) void k_enc_me_cand(uint4 *cand, EncPlanes g, EncRef R, EncRef G, int nmbx, int lambda) {
  enc_me_all<true>(cand, g, R, G, nmbx, lambda);
}

// k_enc_inter_fq reading k_enc_me_all's words; G: GOLD (R's geometry), dclast [ceil(nfrags / 256)][3] (zeroed before)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void k_enc_inter_fq_all(int16_t *levels, int16_t *dcq, uint8_t *cmap, uint32_t *dclast,
                                                          uint32_t *overflow, const int32_t *coded_order, EncPlanes g, EncRef R,
                                                          EncRef G, const uint4 *mb_word, int nmbx, const uint16_t *dequant,
                                                          int64_t n) {
  enc_inter_fq<3>(levels, dcq, cmap, dclast, overflow, coded_order, g, R, G, mb_word, nmbx, dequant, n);
}

// k_enc_inter_dc with three reference classes (dclast [chunks][3])
__global__ __launch_bounds__(256) void k_enc_inter_dc3(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast,
                                                       EncPlanes g, int64_t nfrags) {
  enc_inter_dc<3>(dcr, dcq, cmap, dclast, g, nfrags);
}

// ---- the launches over k_enc_me_all's words (all eight modes, three classes): the overloads of thip_encode_inter.h's --------------
inline hipError_t inter_launch_search(uint4 *mb, const EncPlanes &g, const EncRef &R, const EncRef &G, int nmbx, int nmbs, int lambda,
                                      hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_me_all, dim3((unsigned)nmbs), dim3(256), 0, stream, mb, g, R, G, nmbx, lambda);
  return hipGetLastError();
}

inline hipError_t inter_launch_fq(const InterBufs &o, const int32_t *order, const EncPlanes &g, const EncRef &R, const EncRef &G,
                                  const uint4 *mb, int nmbx, const uint16_t *dequant, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_inter_fq_all, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, stream, o.levels, o.dcq, o.cmap,
                     o.dclast, o.overflow, order, g, R, G, mb, nmbx, dequant, n);
  return hipGetLastError();
}

inline hipError_t inter_launch_dc3(int16_t *dcr, const int16_t *dcq, const uint8_t *cmap, const uint32_t *dclast, const EncPlanes &g,
                                   int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_inter_dc3, dim3((unsigned)((n + kEncChunk - 1) / kEncChunk)), dim3(256), 0, stream, dcr, dcq, cmap, dclast, g, n);
  return hipGetLastError();
}

}  // namespace thip
