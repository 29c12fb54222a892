// thip_activity.h -- oc_mb_activity of one luma block (analyze.c:1152-1237), stated once for the two kernels that compute it:
// k_enc_cost_maps (thip_costmaps.h: all four maps of a frame-size plane) and k_enc_mask_act (thip_encode_mask.h: the activity of the
// encoder's source, read through EncPlanes with the picture clamp).  A lane holds the ten rows around its block as twelve bytes each
// (CmRow: columns -1 .. 10 of the block); how they are fetched is the kernel's own.
//
// With V = up + 2 mid + dn and D = dn - up (column vectors of a row triple) the four edge energies are
//   e1 = sum |V[c+1] - V[c-1]|                e2 = sum |D[c-1] + 2 D[c] + D[c+1]|
//   e3 = sum |2 (dn[c+1] - up[c-1]) + dn[c] - mid[c-1] + mid[c+1] - up[c]|
//   e4 = sum |2 (dn[c-1] - up[c+1]) + dn[c] - mid[c+1] + mid[c-1] - up[c]|
// over the block's 64 positions (analyze.c:1209-1221 with s = block - 1), every term a packed add/sub between a row's "aligned"
// pairs R = {c-1,c0},{c1,c2},... and its "shifted" pairs S = {c0,c1},{c2,c3},...; the logarithm / exponential of the edge
// classification are the reference's integer polynomials (mathops.c:294-314).
#pragma once
#include "thip_device.h"

namespace thip {

// sum |a - b| over one row, added to acc
__device__ __forceinline__ uint32_t sad_row(uint2 a, uint2 b, uint32_t acc) {
  return __builtin_amdgcn_sad_u8(a.y, b.y, __builtin_amdgcn_sad_u8(a.x, b.x, acc));
}
// (the builtin, not inline assembly: the dot instructions have issue hazards against their neighbours that only the compiler
//  can pad when it knows what the instruction is)
__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
__device__ __forceinline__ pk16 pk_abs(pk16 x) {
  const pk16 z = {0, 0};
  return __builtin_elementwise_max(x, z - x);
}
typedef unsigned short upk16 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t sum2_u16(pk16 m, uint32_t acc) {   // acc + m.lo + m.hi, both halves unsigned
  const upk16 one = {(unsigned short)1, (unsigned short)1};
  return __builtin_amdgcn_udot2(__builtin_bit_cast(upk16, m), one, acc, false);
}

// mathops.c:294-314
__device__ __forceinline__ uint32_t cm_bexp32_q10(int z) {
  const int ipart = z >> 10;
  uint32_t n = (uint32_t)(z & 1023) << 4;
  n = (n * ((n * ((n * ((n * 3548u >> 15) + 6817u) >> 15) + 15823u) >> 15) + 22708u) >> 15) + 16384u;
  return 14 - ipart > 0 ? (n + (1u << (13 - ipart))) >> (14 - ipart) : n << (ipart - 14);
}
__device__ __forceinline__ int cm_blog32_q10(uint32_t w) {
  if (w == 0) return -1;
  const int ipart = 32 - __builtin_clz(w);
  const int n = (int)(ipart - 16 > 0 ? w >> (ipart - 16) : w << (16 - ipart)) - 32768 - 16384;
  const int fpart = ((n * ((n * ((n * ((n * -1402 >> 15) + 2546) >> 15) - 5216) >> 15) + 15745)) >> 15) - 6793;
  return (ipart << 10) + (fpart >> 4);
}

// One source row of a luma block as twelve bytes N = columns -1 .. 10 of the block, column -1 in byte 0 (the edge energies read
// columns -1 .. 8: bytes 10 and 11 are never looked at)
struct CmRow {
  uint32_t n0, n1, n2;
};
// the pairs of a row as 16-bit lanes: R[k] = {c(2k-1), c(2k)}, k = 0..4; S[k] = {c(2k), c(2k+1)}, k = 0..3
__device__ __forceinline__ void cm_pairs(const CmRow &r, pk16 R[5], pk16 S[4]) {
  R[0] = as_pk(__builtin_amdgcn_perm(0u, r.n0, 0x0c010c00u));
  R[1] = as_pk(__builtin_amdgcn_perm(0u, r.n0, 0x0c030c02u));
  R[2] = as_pk(__builtin_amdgcn_perm(0u, r.n1, 0x0c010c00u));
  R[3] = as_pk(__builtin_amdgcn_perm(0u, r.n1, 0x0c030c02u));
  R[4] = as_pk(__builtin_amdgcn_perm(0u, r.n2, 0x0c010c00u));
  S[0] = as_pk(__builtin_amdgcn_perm(0u, r.n0, 0x0c020c01u));
  S[1] = as_pk(__builtin_amdgcn_perm(r.n1, r.n0, 0x0c040c03u));
  S[2] = as_pk(__builtin_amdgcn_perm(0u, r.n1, 0x0c020c01u));
  S[3] = as_pk(__builtin_amdgcn_perm(r.n2, r.n1, 0x0c040c03u));
}
__device__ __forceinline__ uint32_t cm_abs_sum(pk16 v, uint32_t acc) { return sum2_u16(pk_abs(v), acc); }

// the block itself out of its rows (rows[1..8]): columns 0..7 = bytes 1..8 of N
__device__ __forceinline__ void cm_block_rows(uint2 (&s)[8], const CmRow (&rows)[10]) {
#pragma unroll
  for (int r = 0; r < 8; r++)
    s[r] = make_uint2(__builtin_amdgcn_alignbyte(rows[r + 1].n1, rows[r + 1].n0, 1u), __builtin_amdgcn_alignbyte(rows[r + 1].n2, rows[r + 1].n1, 1u));
}

// _activity[bi] of oc_mb_activity: 64 x the block's variance, capped where the block is flat, and damped where it is an edge
__device__ __forceinline__ uint32_t cm_block_activity(const CmRow (&rows)[10], const uint2 (&s)[8]) {
  uint32_t x = 0, x2 = 0;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    x = sad_row(s[r], make_uint2(0u, 0u), x);
    x2 = dot4(s[r].x, s[r].x, x2);
    x2 = dot4(s[r].y, s[r].y, x2);
  }
  uint32_t act = (x2 << 6) - x * x;
  if (act < (8u << 12)) {
    act = min(act, 5u << 12);   // the region is flat
  } else {
    uint32_t e1 = 0, e2 = 0, e3 = 0, e4 = 0;
    pk16 Ru[5], Su[4], Rm[5], Sm[4], Rd[5], Sd[4];
    cm_pairs(rows[0], Ru, Su);
    cm_pairs(rows[1], Rm, Sm);
#pragma unroll
    for (int r = 0; r < 8; r++) {
      cm_pairs(rows[r + 2], Rd, Sd);
      pk16 V[5], D[5], Ds[4];
#pragma unroll
      for (int k = 0; k < 5; k++) {
        V[k] = Ru[k] + Rm[k] + Rm[k] + Rd[k];
        D[k] = Rd[k] - Ru[k];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) Ds[k] = Sd[k] - Su[k];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        e1 = cm_abs_sum(V[k + 1] - V[k], e1);
        e2 = cm_abs_sum(D[k] + Ds[k] + Ds[k] + D[k + 1], e2);
        const pk16 t3 = Rd[k + 1] - Ru[k], t4 = Rd[k] - Ru[k + 1];
        e3 = cm_abs_sum(t3 + t3 + Sd[k] - Rm[k] + Rm[k + 1] - Su[k], e3);
        e4 = cm_abs_sum(t4 + t4 + Sd[k] - Rm[k + 1] + Rm[k] - Su[k], e4);
      }
#pragma unroll
      for (int k = 0; k < 5; k++) {
        Ru[k] = Rm[k];
        Rm[k] = Rd[k];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        Su[k] = Sm[k];
        Sm[k] = Sd[k];
      }
    }
    // an edge block when the largest component is at least 40 % of the total (analyze.c:1224-1231)
    if (5u * max(max(e1, e2), max(e3, e4)) > 2u * (e1 + e2 + e3 + e4))
      act = cm_bexp32_q10(0x394A + (7 * (cm_blog32_q10(act) - 0x394A + 5) / 10));
  }
  return act;
}

}  // namespace thip
