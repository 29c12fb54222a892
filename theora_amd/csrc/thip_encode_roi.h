// thip_encode_roi.h -- region-of-interest maps (TH_ENCCTL_THIP_SET_ROI_MAP; the rule is stated in theoraenc_hip.h, "Region of
// interest"): a caller's importance map turned into the scale of every fragment's lambda, alone or on top of activity masking's
// (thip_encode_mask.h).  Two launches in front of the frame's block-qi kernel, behind masking's when masking is on:
//   k_enc_roi_scale  one lane a fragment of any plane: the 8 + 8 map cells of the block's columns and rows (the map is separable),
//                    the sum S of the map over its 64 samples, the exponent e, the ROI scale r and the fragment's final scale to
//                    iscale[fi], on top of masking's scale where there is one.  Three ways to S with one result (roi_frag_sum).
//                    The work group's minimum, maximum and sum of e over its luma fragments and minimum and maximum of the final
//                    scale over all its fragments go to part[blockIdx.x].
//   k_enc_roi_fold   one work group adds the partials up into rec -- no atomics and nothing to zero, so the result does not depend on
//                    scheduling.
// The first part of this file is plain C++ (tests/native/roi_scale_host.cpp runs it lane by lane under AddressSanitizer); the kernels
// and the launch function, which thip_encode.hip's frame and thip_enc_roi_stage both call, follow under __HIPCC__.
#pragma once
#include <stdint.h>

namespace thip {

struct RoiGeo {   // what a lane needs of the frame and the map
  int nh[3], nv[3], froff[3];
  int hdec, vdec;           // chroma's decimation
  int px0, py0, pw, ph;     // the picture region in luma pixels, rows from the top
  int wm, hm;               // the map's size, each 1..16384
  int nfrags;
  int64_t pitch;            // bytes from one map row to the next one down (it may be negative)
};
struct RoiPart {   // a work group of k_enc_roi_scale
  int32_t emin, emax, esum;
  uint32_t imin, imax, pad;
};
struct RoiRec {    // the frame's (32 bytes)
  int32_t exp_min, exp_max;
  int64_t exp_sum;
  uint32_t scale_min, scale_max;
  uint32_t clamped, pad;
};

// 2048 * 2^(f / 16), rounded to nearest
#define THIP_ROI_T {2048, 2139, 2233, 2332, 2435, 2543, 2656, 2774, 2896, 3025, 3158, 3298, 3444, 3597, 3756, 3922}

// the ROI scale (Q11) of the exponent e in -64..64: 2^(-e / 16), in [128, 32768]
__device__ __forceinline__ uint32_t roi_scale(int e) {
  const uint32_t T[16] = THIP_ROI_T;
  const int n = -e, o = n >> 4;
  const uint32_t t = T[n & 15];
  return o >= 0 ? t << o : (t + (1u << (-o - 1))) >> -o;
}

// the fragment's final scale from masking's m (2048 without) and the ROI scale r
__device__ __forceinline__ uint32_t roi_final(uint32_t m, uint32_t r) {
  const uint32_t i = (m * r + 1024u) >> 11;   // (at most 2^30 + 1024)
  return i < 128u ? 128u : i > 32768u ? 32768u : i;
}

// the cell x * n / d: 32-bit where the product fits (the launch function decides)
template <bool kWide>
__device__ __forceinline__ int roi_cell(int x, int n, int d) {
  if (kWide) return (int)((uint64_t)(uint32_t)x * (uint32_t)n / (uint32_t)d);
  return (int)((uint32_t)x * (uint32_t)n / (uint32_t)d);
}

// S of fragment (p, fx, fy) (fy from the bottom): the map summed over the block's 64 samples.
//   coarse   the block's columns fall into at most two cells and so do its rows: at most four loads, weighted by counts;
//   dwords   (the map's base and pitch are 4-byte aligned) the columns span under 8 cells and the dword that holds the last one
//            ends inside the row: up to three aligned dwords a row;
//   bytes    anything else, a map finer than pixels among it: 64 loads.
// No path reads a byte that is not an entry of the map.
template <bool kWide>
__device__ __forceinline__ int roi_frag_sum(const int8_t *map, const RoiGeo &q, bool dwords, int p, int fx, int fy) {
  const int hd = p ? q.hdec : 0, vd = p ? q.vdec : 0;
  int cx[8], cy[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int x = ((fx * 8 + c) << hd) - q.px0, y = ((((q.nv[p] - 1 - fy) * 8) + c) << vd) - q.py0;
    cx[c] = roi_cell<kWide>(x < 0 ? 0 : x > q.pw - 1 ? q.pw - 1 : x, q.wm, q.pw);
    cy[c] = roi_cell<kWide>(y < 0 ? 0 : y > q.ph - 1 ? q.ph - 1 : y, q.hm, q.ph);
  }
  const int spanx = cx[7] - cx[0];   // (the cells do not fall from one sample to the next)
  if (spanx <= 1 && cy[7] - cy[0] <= 1) {
    int nx = 0, ny = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      nx += cx[c] == cx[0];
      ny += cy[c] == cy[0];
    }
    const int8_t *r0 = map + (int64_t)cy[0] * q.pitch, *r1 = map + (int64_t)cy[7] * q.pitch;
    return ny * (nx * (int)r0[cx[0]] + (8 - nx) * (int)r0[cx[7]]) + (8 - ny) * (nx * (int)r1[cx[0]] + (8 - nx) * (int)r1[cx[7]]);
  }
  int S = 0;
  if (dwords && spanx < 8 && (cx[7] | 3) < q.wm) {
    // cx[7] - a0 <= 10: the columns lie in three aligned dwords at the most.  The second and third are loaded where the last column's
    // dword lies when they would lie behind it (the same dword again), so no lane branches and none reads behind its last column
    const int a0 = cx[0] & ~3, last = cx[7] & ~3, a1 = a0 + 4 < last ? a0 + 4 : last, a2 = a0 + 8 < last ? a0 + 8 : last;
    int sh[8], wi[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int k = cx[c] - a0;
      sh[c] = 8 * (k & 3);
      wi[c] = k >> 2;
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int8_t *row = map + (int64_t)cy[r] * q.pitch;
      uint32_t w0, w1, w2;
      __builtin_memcpy(&w0, __builtin_assume_aligned(row + a0, 4), 4);
      __builtin_memcpy(&w1, __builtin_assume_aligned(row + a1, 4), 4);
      __builtin_memcpy(&w2, __builtin_assume_aligned(row + a2, 4), 4);
#pragma unroll
      for (int c = 0; c < 8; c++) S += (int)(int8_t)(uint8_t)((wi[c] == 0 ? w0 : wi[c] == 1 ? w1 : w2) >> sh[c]);
    }
    return S;
  }
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int8_t *row = map + (int64_t)cy[r] * q.pitch;
#pragma unroll
    for (int c = 0; c < 8; c++) S += (int)row[cx[c]];
  }
  return S;
}

// the exponent of the sum S; an entry beyond +-64 (the encoder's own copy of a map has none) cannot carry it outside -64..64
__device__ __forceinline__ int roi_exponent(int S) {
  const int e = (S + 32) >> 6;
  return e < -64 ? -64 : e > 64 ? 64 : e;
}

// the lane of fragment fi: its plane and exponent, and its final scale; mask: masking's scales or nullptr
template <bool kWide>
__device__ __forceinline__ uint32_t roi_lane(const int8_t *map, const uint16_t *mask, const RoiGeo &q, bool dwords, int fi, int &p, int &e) {
  p = fi >= q.froff[2] ? 2 : fi >= q.froff[1] ? 1 : 0;
  const int loc = fi - q.froff[p], fy = loc / q.nh[p], fx = loc - fy * q.nh[p];
  e = roi_exponent(roi_frag_sum<kWide>(map, q, dwords, p, fx, fy));
  return roi_final(mask ? (uint32_t)mask[fi] : 2048u, roi_scale(e));
}

inline int roi_parts(int64_t nfrags) { return (int)((nfrags + 255) / 256); }

}  // namespace thip

#ifdef __HIPCC__
#include "thip_encode.h"

namespace thip {

// the work group's (256 lanes) minima, maxima and sum, in every lane
__device__ __forceinline__ void roi_group_fold(int &emin, int &emax, int64_t &esum, uint32_t &imin, uint32_t &imax) {
  __shared__ int s_e[2][4];
  __shared__ uint32_t s_i[2][4];
  __shared__ int64_t s_sum[4];
  int lo = (int)(uint32_t)esum, hi = (int)(uint32_t)((uint64_t)esum >> 32);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    emin = min(emin, __shfl_xor(emin, m));
    emax = max(emax, __shfl_xor(emax, m));
    imin = min(imin, (uint32_t)__shfl_xor((int)imin, m));
    imax = max(imax, (uint32_t)__shfl_xor((int)imax, m));
    const uint32_t l = (uint32_t)__shfl_xor(lo, m), h = (uint32_t)__shfl_xor(hi, m);
    esum += (int64_t)((uint64_t)h << 32 | l);
    lo = (int)(uint32_t)esum;
    hi = (int)(uint32_t)((uint64_t)esum >> 32);
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = (int)threadIdx.x >> 6;
    s_e[0][w] = emin;
    s_e[1][w] = emax;
    s_i[0][w] = imin;
    s_i[1][w] = imax;
    s_sum[w] = esum;
  }
  __syncthreads();
  emin = min(min(s_e[0][0], s_e[0][1]), min(s_e[0][2], s_e[0][3]));
  emax = max(max(s_e[1][0], s_e[1][1]), max(s_e[1][2], s_e[1][3]));
  imin = min(min(s_i[0][0], s_i[0][1]), min(s_i[0][2], s_i[0][3]));
  imax = max(max(s_i[1][0], s_i[1][1]), max(s_i[1][2], s_i[1][3]));
  esum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// iscale [nfrags]: the final scales; mask [nfrags]: masking's, or nullptr (it may be iscale itself: a lane reads its entry before it
// writes it); part [roi_parts(nfrags)]
template <bool kWide>
__global__ __launch_bounds__(256) void k_enc_roi_scale(uint16_t *iscale, RoiPart *part, const int8_t *map, const uint16_t *mask, RoiGeo q,
                                                       int dwords) {
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);
  const bool live = u < q.nfrags;
  const int fi = min(u, q.nfrags - 1);   // (a lane past the last fragment: the last one's, it stores and adds nothing)
  int p, e;
  const uint32_t i = roi_lane<kWide>(map, mask, q, dwords != 0, fi, p, e);
  if (live) iscale[u] = (uint16_t)i;
  const bool luma = live && p == 0;
  int emin = luma ? e : 65, emax = luma ? e : -65;
  int64_t esum = luma ? e : 0;
  uint32_t imin = live ? i : 0xFFFFFFFFu, imax = live ? i : 0u;
  roi_group_fold(emin, emax, esum, imin, imax);
  if (threadIdx.x == 0) part[blockIdx.x] = RoiPart{emin, emax, (int32_t)esum, imin, imax, 0u};
}

// rec [1] from part [npart]; clamped: the count the map's copy left (the encoder's), or nullptr: 0
__global__ __launch_bounds__(256) void k_enc_roi_fold(RoiRec *rec, const RoiPart *part, int npart, const uint32_t *clamped) {
  int emin = 65, emax = -65;
  int64_t esum = 0;
  uint32_t imin = 0xFFFFFFFFu, imax = 0u;
  for (int k = (int)threadIdx.x; k < npart; k += 256) {
    emin = min(emin, part[k].emin);
    emax = max(emax, part[k].emax);
    esum += part[k].esum;
    imin = min(imin, part[k].imin);
    imax = max(imax, part[k].imax);
  }
  roi_group_fold(emin, emax, esum, imin, imax);
  if (threadIdx.x == 0) *rec = RoiRec{emin, emax, esum, imin, imax, clamped ? *clamped : 0u, 0u};
}

// the encoder's own copy of a caller's device map: dst [hm][wm] tight, every entry clamped to +-64, and how many were beyond it
// added to *clamped (which the caller zeroed on the same stream; an integer sum does not depend on the order)
__global__ __launch_bounds__(256) void k_enc_roi_copy(int8_t *dst, uint32_t *clamped, const int8_t *src, int64_t pitch, int wm, int hm) {
  const int64_t n = (int64_t)wm * hm;
  uint32_t bad = 0;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
    const int y = (int)(k / wm), x = (int)(k - (int64_t)y * wm);
    const int v = src[(int64_t)y * pitch + x], c = min(max(v, -64), 64);
    bad += c != v;
    dst[k] = (int8_t)c;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) bad += (uint32_t)__shfl_xor((int)bad, m);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(clamped, bad);
}

inline hipError_t roi_launch_copy(int8_t *dst, uint32_t *clamped, const int8_t *src, int64_t pitch, int wm, int hm, hipStream_t stream) {
  const int64_t n = (int64_t)wm * hm;
  hipError_t err = hipMemsetAsync(clamped, 0, 4, stream);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_enc_roi_copy, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, stream, dst, clamped, src, pitch, wm, hm);
  return hipGetLastError();
}

// every fragment's final scale from the map [hm][wm] at pitch: iscale [n]; mask: masking's scales [n] (iscale itself will do) or
// nullptr; part [roi_parts(n)], rec [1]; clamped as k_enc_roi_fold takes it
inline hipError_t roi_launch_scale(uint16_t *iscale, const uint16_t *mask, RoiPart *part, RoiRec *rec, const int8_t *map, int wm, int hm,
                                   int64_t pitch, const uint32_t *clamped, const EncPlanes &g, int64_t n, hipStream_t stream) {
  RoiGeo q;
  for (int p = 0; p < 3; p++) {
    q.nh[p] = g.nh[p];
    q.nv[p] = g.nv[p];
    q.froff[p] = g.froff[p];
  }
  q.hdec = g.nh[1] != g.nh[0];
  q.vdec = g.nv[1] != g.nv[0];
  q.px0 = g.px0[0];
  q.py0 = g.py0[0];
  q.pw = g.pw[0];
  q.ph = g.ph[0];
  q.wm = wm;
  q.hm = hm;
  q.nfrags = (int)n;
  q.pitch = pitch;
  const bool wide = (uint64_t)(q.pw - 1) * (uint64_t)wm >> 32 || (uint64_t)(q.ph - 1) * (uint64_t)hm >> 32;
  const int dwords = (((uintptr_t)map | (uintptr_t)pitch) & 3) == 0;
  const dim3 grid((unsigned)roi_parts(n)), wg(256);
  if (wide) hipLaunchKernelGGL(k_enc_roi_scale<true>, grid, wg, 0, stream, iscale, part, map, mask, q, dwords);
  else hipLaunchKernelGGL(k_enc_roi_scale<false>, grid, wg, 0, stream, iscale, part, map, mask, q, dwords);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_enc_roi_fold, dim3(1), wg, 0, stream, rec, (const RoiPart *)part, roi_parts(n), clamped);
  return hipGetLastError();
}

}  // namespace thip
#endif
