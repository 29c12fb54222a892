// thip_fdct.h -- the forward DCT and the fused transform + quantiser core shared by thip_slots.hip (the batched
// oc_enc_fdct8x8 / oc_enc_quantize slots) and thip_encode.hip (the intra encoder's device stage).
#pragma once
#include "thip_device.h"

namespace thip {

// 1-D forward DCT, in place (the arithmetic of lib/fdct.c:28-120, whose rounding constants make the
// transform the exact inverse partner of the decoder's; outputs truncate to int16 where the reference stores
// into ogg_int16_t).  Written as the three kinds of step it consists of:
//   fd_scale(v, bias)        v * (1 + 27146/65536) rounded with `bias`, nudged away from zero: the sqrt(2)-ish
//                            scalings of the even part and of the two middle odd terms;
//   fd_rot(a, b, ca, cb, k)  the first output of a plane rotation, (ca*a + cb*b + k) >> 16, nudged by b != 0;
//   fd_back(u, c, x, m, k, s) the second output recovered from the first: r = +-(c*u >> 16 - x), then
//                            r * (1 + m / 2^s) rounded with k, nudged away from zero.
__device__ __forceinline__ int fd_nz(int v) { return v != 0 ? 1 : 0; }
__device__ __forceinline__ int fd_scale(int v, int bias) { return ((27146 * v + bias) >> 16) + v + fd_nz(v); }
__device__ __forceinline__ int fd_rot(int a, int b, int ca, int cb, int k) { return ((ca * a + cb * b + k) >> 16) + fd_nz(b); }
__device__ __forceinline__ int fd_back(int r, int m, int k, int s) { return ((r * m + k) >> s) + r + fd_nz(r); }
__device__ __forceinline__ void fdct8(int &x0, int &x1, int &x2, int &x3, int &x4, int &x5, int &x6,
                                      int &x7) {
  // stage 1: mirror sums and differences; stage 2: the even half folds once more
  const int s07 = x0 + x7, d07 = x0 - x7, s16 = x1 + x6, d16 = x1 - x6;
  const int s25 = x2 + x5, d25 = x2 - x5, s34 = x3 + x4, d34 = x3 - x4;
  const int e0 = s07 + s34, e3 = s07 - s34, e1 = s16 + s25, e2 = s16 - s25;
  // even outputs 0 and 4 (fdct.c:96-100), 2 and 6 (fdct.c:102-106)
  const int p = ((27146 * e0 + 0x4000) >> 16) + e0 + fd_nz(e0), q = fd_scale(e1, 0xB500);
  const int y0 = (p + q) >> 1, y4 = p - y0;
  const int y2 = fd_rot(e2, e3, kC6, kC2, 0x6CB7);
  const int y6 = fd_back(((kC6 * y2) >> 16) - e2, 21600, 0x2800, 18);
  // odd half: the two middle differences are rotated by pi/4 first (fdct.c:87-93)
  const int ms = d16 + d25, md = d16 - d25;
  const int h5 = fd_scale(md, 0xB500) >> 1, h6 = fd_scale(ms, 0xB500) >> 1;
  const int o4 = d34 + h5, o5 = d34 - h5, o7 = d07 + h6, o6 = d07 - h6;
  // odd outputs 5 and 3 (fdct.c:108-112), 1 and 7 (fdct.c:114-118)
  const int y5 = fd_rot(o6, o5, kC5, kC3, 0x0E3D);
  const int y3 = fd_back(o6 - ((kC5 * y5) >> 16), 26568, 0x3400, 17);
  const int y1 = fd_rot(o4, o7, kC7, kC1, 0x7B1B);
  const int y7 = fd_back(((kC7 * y1) >> 16) - o4, 20539, 0x3000, 20);
  x0 = sx16(y0); x1 = sx16(y1); x2 = sx16(y2); x3 = sx16(y3);
  x4 = sx16(y4); x5 = sx16(y5); x6 = sx16(y6); x7 = sx16(y7);
}

// natural position of zig-zag index i -- lib/internal.c:27 (first 64 entries)
__device__ constexpr int kFZigZag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};


// The transform-and-quantise core of k_enc_intra_fq (thip_encode.h), in the layout of k_enc_fdct_quantize4 (thip_slots.hip) -- four
// lanes a block, lane 4b + j of the wave working on block b (b = lane >> 2, j = lane & 3).  k_enc_fdct_quantize4 keeps its own inline
// copy, which also writes the unquantised coefficients and the last non-zero index: calling this function from it cost its resource
// line an SGPR.  On entry the wave's 2 KB `lds` holds the sixteen blocks' int16 input, piece pc (row pc, natural order) of block bb at
// lds[bb * 8 + ((pc + bb) & 7)], and s_t the block's 64 table entries by natural position (step | reciprocal m << 16, shift l |
// zig-zag index << 8); a barrier lies behind both.  On return the same 2 KB hold the block's quantised levels in zig-zag order, in the
// same layout, every LDS operation of the wave complete.  rate_fdct4_lds (thip_rate.h) copies the transform half: a fix here belongs
// there too.
__device__ __forceinline__ void fdct_quantize4_lds(int4 *lds, const uint2 *s_t, int b, int j) {
  const int *ldw = reinterpret_cast<const int *>(lds);
  int c0[8], c1[8];   // columns 2j and 2j + 1
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int w = ldw[(b * 8 + ((r + b) & 7)) * 4 + j];
    c0[r] = sx16(sx16(w) << 2);                          // fdct.c:136
    c1[r] = sx16((w >> 16) << 2);
  }
  if (j == 0) {                                          // fdct.c:139-141: positions 0, 1 and 8
    c0[0] = sx16(c0[0] + (c0[0] != 0) + 1);
    c1[0] = sx16(c1[0] + 1);
    c0[1] = sx16(c0[1] - 1);
  }
  fdct8(c0[0], c0[1], c0[2], c0[3], c0[4], c0[5], c0[6], c0[7]);
  fdct8(c1[0], c1[1], c1[2], c1[3], c1[4], c1[5], c1[6], c1[7]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // every lane of the wave has read the input
  int *ldww = reinterpret_cast<int *>(lds);
#pragma unroll
  for (int k = 0; k < 8; k++) ldww[(b * 8 + ((k + b) & 7)) * 4 + j] = (c0[k] & 0xFFFF) | (c1[k] << 16);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int o[16];           // rows 2j and 2j + 1, natural position (2j + h) * 8 + c at o[h * 8 + c]
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int r = 2 * j + h;
    const int4 w = lds[b * 8 + ((r + b) & 7)];
    int v[8] = {sx16(w.x), w.x >> 16, sx16(w.y), w.y >> 16, sx16(w.z), w.z >> 16, sx16(w.w), w.w >> 16};
    fdct8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
#pragma unroll
    for (int c = 0; c < 8; c++) o[h * 8 + c] = sx16((v[c] + 2) >> 2);   // fdct.c:149
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int16_t *lds16 = reinterpret_cast<int16_t *>(lds);
  // where zig-zag index z of block b lies in the wave's area (the same rotation of 16-byte pieces)
  auto at = [&](int z) { return (b * 8 + (((z >> 3) + b) & 7)) * 8 + (z & 7); };
  // (the table entries of positions k, k + 1: one 16-byte read)
  auto entries = [&](int k) { return *reinterpret_cast<const uint4 *>(&s_t[(2 * j + (k >> 3)) * 8 + (k & 7)]); };
#pragma unroll
  for (int k = 0; k < 16; k += 2) {   // enquant.c:228-245
    const uint4 e = entries(k);
#pragma unroll
    for (int h2 = 0; h2 < 2; h2++) {
      const uint32_t ex = h2 ? e.z : e.x, ey = h2 ? e.w : e.y;
      const int z = (int)(ey >> 8), d = (int)(ex & 0xFFFFu), m = (int)ex >> 16, l = (int)(ey & 0xFFu);
      int val = o[k + h2] << 1, q = 0;
      if (abs(val) >= d) {
        const int sg = val >> 31;
        val += (d + sg) ^ sg;
        q = sx16(((((m * val) >> 16) + val) >> l) - sg);
      }
      lds16[at(z)] = (int16_t)q;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

}  // namespace thip
