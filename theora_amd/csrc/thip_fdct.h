// thip_fdct.h -- the forward DCT (lib/fdct.c) and the quantiser (lib/enquant.c), each stated once, for every kernel that
// transforms or quantises: the batched oc_enc_fdct8x8 / oc_enc_quantize slots (thip_slots.hip), the th_encode_* transform kernels
// (thip_encode.h, thip_encode_inter.h, thip_encode_bqi.h) and the rate probe (thip_rate.h).
//
//   fdct8                                    the 1-D transform
//   quant_recip, quant_level                 oc_iquant_init and a coefficient through oc_enc_quantize
//   quant_entry, quant_entry_fields          the 8-byte table entry of the four-lane kernels, packed and taken apart
//   fdct8x8_lane, quant_tables, quantize_lane    one block a lane
//   lds_block_piece, lds_block_at, wave_blocks_in / _out / _out_of, wave_lds_handover
//                                            four lanes a block: the wave's sixteen blocks in its 2 KB of LDS
//   fdct4_lds, lane_entries4, quantize4_lds, fdct_quantize4_lds
//                                            ... their transform, a lane's table entries, its quantising pass, both halves
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

// ---- the quantiser ---------------------------------------------------------------------------------------------------------------

// oc_iquant_init (enquant.c:183-191) for the doubled step d2 = dequant << 1 (not zero): l is the bit length of d2 less one, m the
// reciprocal 2^(16 + l) / d2 + 1 less 2^16, as an int16
__host__ __device__ __forceinline__ void quant_recip(uint32_t d2, int &m, int &l) {
  l = 31 - __builtin_clz(d2);                                // OC_ILOGNZ_32(d2) - 1
  const uint32_t t = 1u + ((1u << (16 + l)) / d2);
  m = (int)(int16_t)(t - 0x10000u);
}

// one coefficient through oc_enc_quantize (enquant.c:228-245) with the step d and its reciprocal {m, l}: its level.  passed() is
// called when it is not below the threshold -- the reference's `nonzero` is the last index at which that happened
template <class Passed>
__device__ __forceinline__ int quant_level(int coef, int d, int m, int l, Passed &&passed) {
  int val = coef << 1, lv = 0;
  if (abs(val) >= d) {
    const int sg = val >> 31;
    val += (d + sg) ^ sg;
    lv = sx16(((((m * val) >> 16) + val) >> l) - sg);
    passed();
  }
  return lv;
}

// A table entry of the four-lane kernels, 8 bytes: step | reciprocal m << 16, shift l | zig-zag index << 8.
struct QuantEntry {
  int d, m, l, z;
};
__host__ __device__ __forceinline__ uint2 quant_entry(uint32_t dq, int m, int l, int z) {
  return make_uint2(dq | (uint32_t)(uint16_t)m << 16, (uint32_t)(l & 0xFF) | (uint32_t)z << 8);
}
__device__ __forceinline__ QuantEntry quant_entry_fields(uint32_t ex, uint32_t ey) {
  return {(int)(ex & 0xFFFFu), (int)ex >> 16, (int)(ey & 0xFFu), (int)(ey >> 8)};
}

// the reciprocal of the step at zig-zag index z: the caller's when it hands in a table (oc_iquant {m, l} pairs, enquant.h; what
// thip_enc_enquant_table_init builds), else derived here
__device__ __forceinline__ void quant_recip_at(const uint16_t *dequant, const int16_t *enquant, int z, int &m, int &l) {
  if (enquant) {
    m = (int)enquant[2 * z];
    l = (int)enquant[2 * z + 1];
  } else {
    quant_recip((uint32_t)dequant[z] << 1, m, l);
  }
}

// ---- one block a lane ------------------------------------------------------------------------------------------------------------

// oc_enc_fdct8x8 (fdct.c:128-150) on the block in w (natural order; w is used up): the coefficients in zig-zag order in o
__device__ __forceinline__ void fdct8x8_lane(int w[64], int o[64]) {
#pragma unroll
  for (int k = 0; k < 64; k++) w[k] = sx16(w[k] << 2);        // fdct.c:136
  w[0] = sx16(w[0] + (w[0] != 0) + 1);                        // fdct.c:139-141
  w[1] = sx16(w[1] + 1);
  w[8] = sx16(w[8] - 1);
  // columns of w -> rows of z (fdct.c:143), then columns of z -> rows of w (fdct.c:145).
  // In registers: transform each column in place (result element k of column c sits at
  // [k][c], i.e. z transposed), then each row in place; the final element (r,c) holds
  // what the reference leaves at w[r*8+c] transposed twice == natural position.
#pragma unroll
  for (int c = 0; c < 8; c++)
    fdct8(w[0 * 8 + c], w[1 * 8 + c], w[2 * 8 + c], w[3 * 8 + c], w[4 * 8 + c], w[5 * 8 + c], w[6 * 8 + c], w[7 * 8 + c]);
#pragma unroll
  for (int r = 0; r < 8; r++)
    fdct8(w[r * 8 + 0], w[r * 8 + 1], w[r * 8 + 2], w[r * 8 + 3], w[r * 8 + 4], w[r * 8 + 5], w[r * 8 + 6], w[r * 8 + 7]);
#pragma unroll
  for (int k = 0; k < 64; k++) o[k] = sx16((w[kFZigZag[k]] + 2) >> 2);   // fdct.c:149
}

// the work group's step, reciprocal and shift by zig-zag index, filled by its first 64 threads; a barrier belongs behind it
__device__ __forceinline__ void quant_tables(int *s_d, int *s_m, int *s_l, const uint16_t *dequant, const int16_t *enquant) {
  if (threadIdx.x < 64) {
    const int z = (int)threadIdx.x;
    s_d[z] = (int)dequant[z];
    quant_recip_at(dequant, enquant, z, s_m[z], s_l[z]);
  }
}

// oc_enc_quantize (enquant.c:219-248) on the block in v (zig-zag order), in place; returns its `nonzero`
__device__ __forceinline__ int quantize_lane(int v[64], const int *s_d, const int *s_m, const int *s_l) {
  int nz = 0;
#pragma unroll
  for (int z = 0; z < 64; z++) v[z] = quant_level(v[z], s_d[z], s_m[z], s_l[z], [&] { nz = z; });
  return nz;
}

// ---- four lanes a block, sixteen blocks a wave -----------------------------------------------------------------------------------
// Lane 4b + j of the wave works on block b (b = lane >> 2, j = lane & 3).  The wave's 2 KB of LDS hold its sixteen blocks as int16,
// eight 16-byte pieces each (a row in natural order, or eight indices of the zig-zag order), piece pc of block bb ROTATED to
// lds[bb * 8 + ((pc + bb) & 7)], so that sixteen blocks' equal pieces spread over the banks.

__device__ __forceinline__ int lds_block_piece(int bb, int pc) { return bb * 8 + ((pc + bb) & 7); }
// ... and value z of block b as an int16 index
__device__ __forceinline__ int lds_block_at(int b, int z) { return lds_block_piece(b, z >> 3) * 8 + (z & 7); }

// Between one lane's LDS stores and another lane's loads of them (and between loads and the stores that overwrite them) inside a
// wave: the wave's LDS operations complete in order, so waiting for them is enough; the wave barrier emits no instruction and keeps
// the compiler from moving LDS operations of the two sides across the wait.  No other wave touches these 2 KB.
__device__ __forceinline__ void wave_lds_handover() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The wave's sixteen blocks (b0 .. b0 + 15 of the n in g, 128 bytes each) between memory and LDS, coalesced: two 16-byte pieces a
// lane.  _out_of: block bb's pieces come from src(bb), a 2 KB area in the layout above.  Blocks past the last move nothing.
__device__ __forceinline__ void wave_blocks_in(int4 *lds, const int16_t *g, int64_t b0, int64_t n) {
  const int lane = (int)threadIdx.x & 63;
  const int4 *gp = reinterpret_cast<const int4 *>(g) + b0 * 8;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int idx = q * 64 + lane, bb = idx >> 3, pc = idx & 7;
    if (b0 + bb < n) lds[lds_block_piece(bb, pc)] = gp[idx];
  }
}
template <class Src>
__device__ __forceinline__ void wave_blocks_out_of(int16_t *g, Src &&src, int64_t b0, int64_t n) {
  const int lane = (int)threadIdx.x & 63;
  int4 *gp = reinterpret_cast<int4 *>(g) + b0 * 8;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const int idx = q * 64 + lane, bb = idx >> 3, pc = idx & 7;
    const int4 *s = src(bb);
    if (b0 + bb < n) gp[idx] = s[lds_block_piece(bb, pc)];
  }
}
__device__ __forceinline__ void wave_blocks_out(int16_t *g, const int4 *lds, int64_t b0, int64_t n) {
  wave_blocks_out_of(g, [=](int) { return lds; }, b0, n);
}

// oc_enc_fdct8x8 (fdct.c:128-150) on block b by its four lanes.  On entry `lds` holds the sixteen blocks' int16 input, piece = row, and
// the stores that put it there are complete (a barrier, or wave_lds_handover).  The lane takes columns 2j, 2j + 1 for the first pass
// (fdct.c:143), the block is transposed through the same 2 KB as int16 pairs, the lane takes rows 2j, 2j + 1 for the second
// (fdct.c:145).  On return o[h * 8 + c] holds natural position (2j + h) * 8 + c, and the wave is done with the LDS: it may be
// overwritten.
__device__ __forceinline__ void fdct4_lds(int4 *lds, int b, int j, int o[16]) {
  int *ldw = reinterpret_cast<int *>(lds);
  int c0[8], c1[8];   // columns 2j and 2j + 1
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int w = ldw[lds_block_piece(b, r) * 4 + j];
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
  wave_lds_handover();                                   // every lane of the wave has read the input
#pragma unroll
  for (int k = 0; k < 8; k++) ldw[lds_block_piece(b, k) * 4 + j] = (c0[k] & 0xFFFF) | (c1[k] << 16);
  wave_lds_handover();
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int4 w = lds[lds_block_piece(b, 2 * j + h)];
    int v[8] = {sx16(w.x), w.x >> 16, sx16(w.y), w.y >> 16, sx16(w.z), w.z >> 16, sx16(w.w), w.w >> 16};
    fdct8(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
#pragma unroll
    for (int c = 0; c < 8; c++) o[h * 8 + c] = sx16((v[c] + 2) >> 2);   // fdct.c:149
  }
  wave_lds_handover();
}

// f(k, entry) for the lane's sixteen natural positions (2j + (k >> 3)) * 8 + (k & 7), k = 0..15, from s_t: the block's 64 table
// entries BY NATURAL POSITION -- two runs of eight entries a lane, read sixteen bytes (two entries) at a time
template <class F>
__device__ __forceinline__ void lane_entries4(const uint2 *s_t, int j, F &&f) {
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    const uint4 e = *reinterpret_cast<const uint4 *>(&s_t[(2 * j + (k >> 3)) * 8 + (k & 7)]);
    f(k, quant_entry_fields(e.x, e.y));
    f(k + 1, quant_entry_fields(e.z, e.w));
  }
}

// The lane's sixteen coefficients o (as fdct4_lds leaves them) through the quantiser; the levels go to `lds` in ZIG-ZAG order (the
// layout above, piece = eight indices), and hook(z, coefficient, level, step) sees each.  Returns the largest index that passed the
// threshold among the sixteen (0: none).  The caller hands over (wave_lds_handover) before other lanes read the levels.
template <class Hook>
__device__ __forceinline__ int quantize4_lds(int4 *lds, const uint2 *s_t, int b, int j, const int o[16], Hook &&hook) {
  int16_t *lds16 = reinterpret_cast<int16_t *>(lds);
  int nz = 0;
  lane_entries4(s_t, j, [&](int k, const QuantEntry &e) {
    const int lv = quant_level(o[k], e.d, e.m, e.l, [&] { nz = max(nz, e.z); });
    lds16[lds_block_at(b, e.z)] = (int16_t)lv;
    hook(e.z, o[k], lv, e.d);
  });
  return nz;
}

// The transform-and-quantise core of k_enc_intra_fq and enc_inter_fq: fdct4_lds's contract on entry, and a barrier behind s_t too.
// On return the same 2 KB hold the blocks' quantised levels in zig-zag order, every LDS operation of the wave complete.
__device__ __forceinline__ void fdct_quantize4_lds(int4 *lds, const uint2 *s_t, int b, int j) {
  int o[16];
  fdct4_lds(lds, b, j, o);
  quantize4_lds(lds, s_t, b, j, o, [](int, int, int, int) {});
  wave_lds_handover();
}

}  // namespace thip
