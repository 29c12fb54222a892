// thip_encode_mask.h -- activity masking (TH_ENCCTL_THIP_SET_MASKING; the rule is stated in theoraenc_hip.h, "Activity masking"): a
// scale a block for the lambda of the block-qi choice (thip_encode_bqi.h), from the activity of the frame's source.  Two launches in
// front of the quantising kernel, and the masked forms of the three block-qi kernels:
//   k_enc_mask_act    one lane a luma block: oc_mb_activity's value of the block (cm_block_activity of thip_activity.h, the body
//                     k_enc_cost_maps runs) over the source as the block kernels see it -- the picture region, clamped outward
//                     (enc_src_block's clamp) -- to act[fi] (fragment raster order, rows from the bottom as everywhere in the
//                     bitstream), and the work group's sum and maximum to part[blockIdx.x].
//   k_enc_mask_scale  one lane a fragment of any plane.  Every work group adds the partials up itself (a few hundred at 4K) and
//                     forms the frame average A -- no atomics and nothing to zero, so the result does not depend on scheduling --,
//                     then each lane writes its fragment's scale (Q11) to iscale[fi]; a chroma lane forms its macro block's four
//                     luma scales again instead of waiting for them.  Work group 0 writes A and the maximum activity to rec.
// The launch functions sit beside the kernels; thip_encode.hip's frame and thip_enc_mask_stage call the same ones.
#pragma once
#include "thip_activity.h"
#include "thip_encode_bqi.h"

namespace thip {

struct MaskPart {   // a work group of k_enc_mask_act
  uint64_t sum;
  uint32_t max, pad;
};
struct MaskRec {    // the frame's: A (the average, floored at 64) and the maximum activity
  uint64_t avg, max;
};

constexpr int kMaskFloor = 64;   // A's floor

__device__ __forceinline__ uint64_t mask_shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return (uint64_t)hi << 32 | lo;
}
// the work group's (256 lanes) sum and maximum, in every lane
__device__ __forceinline__ void mask_group_sum_max(uint64_t &sum, uint32_t &mx) {
  __shared__ uint64_t s_sum[4];
  __shared__ uint32_t s_max[4];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    sum += mask_shfl_xor64(sum, m);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, m));
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    s_max[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
  mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
}

// act [nluma], part [ceil(nluma / 256)]
__global__ __launch_bounds__(256) void k_enc_mask_act(uint32_t *act, MaskPart *part, EncPlanes g, int nluma) {
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);
  const bool live = u < nluma;
  const int fi = min(u, nluma - 1);   // (a lane past the last block: the last block's, it stores and adds nothing)
  const int nh = g.nh[0], fy = fi / nh, fx = fi - fy * nh;
  // in the picture's coordinates, rows from the top: the block's left column and top row, and the picture's last column and row.
  // A coordinate clamped into the frame and then into the picture is the coordinate clamped into the picture.
  const int x0 = fx * 8 - g.px0[0], y0 = (g.nv[0] - 1 - fy) * 8 - g.py0[0], pw1 = g.pw[0] - 1, ph1 = g.ph[0] - 1;
  const uint8_t *src = g.src[0];
  const int64_t stride = g.stride[0];
  CmRow rows[10];
  // Three ways to twelve bytes a row (no alignment is promised) that never read outside the picture: the block's columns -1 .. 10
  // as they are (inside); columns 0 .. 11 with column 0 doubled (the block starts at the picture's left edge); columns -4 .. 7
  // with column 7 doubled (it ends at the right edge).  Any other block -- the picture's edge cuts through it or it lies outside,
  // which takes a picture region that is not a whole number of blocks -- gathers its bytes one by one.
  const int mode = x0 >= 1 && x0 + 10 <= pw1 ? 0 : x0 == 0 && pw1 >= 11 ? 1 : x0 + 7 == pw1 && x0 >= 4 ? 2 : 3;
  if (mode != 3) {
    const int xs = mode == 0 ? x0 - 1 : mode == 1 ? 0 : x0 - 4;
#pragma unroll
    for (int r = 0; r < 10; r++) {
      const uint8_t *row = src + (int64_t)min(max(y0 - 1 + r, 0), ph1) * stride + xs;
      uint32_t w[3];
      __builtin_memcpy(w, row, 12);
      const uint32_t l0 = w[0] << 8 | (w[0] & 0xFFu), l1 = __builtin_amdgcn_alignbyte(w[1], w[0], 3u);
      const uint32_t m2 = __builtin_amdgcn_alignbyte(w[2], w[1], 3u), r2 = w[2] >> 24;
      rows[r].n0 = mode == 0 ? w[0] : mode == 1 ? l0 : l1;
      rows[r].n1 = mode == 0 ? w[1] : mode == 1 ? l1 : m2;
      rows[r].n2 = mode == 0 ? w[2] : mode == 1 ? m2 : (r2 << 8 | r2);
    }
  } else {
    int cx[10];
#pragma unroll
    for (int c = 0; c < 10; c++) cx[c] = min(max(x0 - 1 + c, 0), pw1);
#pragma unroll
    for (int r = 0; r < 10; r++) {
      const uint8_t *row = src + (int64_t)min(max(y0 - 1 + r, 0), ph1) * stride;
      rows[r].n0 = (uint32_t)row[cx[0]] | (uint32_t)row[cx[1]] << 8 | (uint32_t)row[cx[2]] << 16 | (uint32_t)row[cx[3]] << 24;
      rows[r].n1 = (uint32_t)row[cx[4]] | (uint32_t)row[cx[5]] << 8 | (uint32_t)row[cx[6]] << 16 | (uint32_t)row[cx[7]] << 24;
      rows[r].n2 = (uint32_t)row[cx[8]] | (uint32_t)row[cx[9]] << 8;
    }
  }
  uint2 s[8];
  cm_block_rows(s, rows);
  const uint32_t a = cm_block_activity(rows, s);
  if (live) act[u] = a;
  uint64_t sum = live ? a : 0u;
  uint32_t mx = live ? a : 0u;
  mask_group_sum_max(sum, mx);
  if (threadIdx.x == 0) part[blockIdx.x] = MaskPart{sum, mx, 0u};
}

// the luma scale of activity a against the average A with ratio k, Q11: in [2048 / k, 2048 k]
__host__ __device__ __forceinline__ uint32_t mask_scale(uint64_t a, uint64_t A, uint64_t k) {
  const uint64_t den = a + k * A;
  return (uint32_t)((2048u * (k * a + A) + den / 2) / den);
}
// the chroma scale of a macro block with the luma scales i[0..3]: the least of them when none lies under 2048, else the second
// least, and never under 2048
__host__ __device__ __forceinline__ uint32_t mask_chroma_scale(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3) {
  uint32_t lo0 = i0 < i1 ? i0 : i1, hi0 = i0 < i1 ? i1 : i0, lo1 = i2 < i3 ? i2 : i3, hi1 = i2 < i3 ? i3 : i2;
  const uint32_t least = lo0 < lo1 ? lo0 : lo1, mid = lo0 < lo1 ? lo1 : lo0, hi = hi0 < hi1 ? hi0 : hi1;
  const uint32_t second = mid < hi ? mid : hi;
  const uint32_t m = least >= 2048u ? least : second;
  return m > 2048u ? m : 2048u;
}

// iscale [nfrags], rec [1]; act, part as k_enc_mask_act left them (npart = its work groups)
__global__ __launch_bounds__(256) void k_enc_mask_scale(uint16_t *iscale, MaskRec *rec, const uint32_t *act, const MaskPart *part,
                                                        int npart, EncPlanes g, int nfrags, int k) {
  uint64_t sum = 0;
  uint32_t mx = 0;
  for (int i = (int)threadIdx.x; i < npart; i += 256) {
    sum += part[i].sum;
    mx = max(mx, part[i].max);
  }
  mask_group_sum_max(sum, mx);
  const uint64_t nluma = (uint64_t)g.nh[0] * (uint64_t)g.nv[0];
  const uint64_t mean = (sum + nluma / 2) / nluma, A = mean > (uint64_t)kMaskFloor ? mean : (uint64_t)kMaskFloor;
  if (blockIdx.x == 0 && threadIdx.x == 0) *rec = MaskRec{A, mx};
  const int fi = (int)(blockIdx.x * 256 + threadIdx.x);
  if (fi >= nfrags) return;
  int p, fx, fy;
  enc_frag_xy(g, fi, p, fx, fy);
  if (p == 0) {
    iscale[fi] = (uint16_t)mask_scale(act[fi], A, (uint64_t)k);
    return;
  }
  // the chroma fragment's macro block: its four luma blocks (a plane that is not decimated has two fragments a macro block there)
  const int bx = (g.nh[1] != g.nh[0] ? fx : fx >> 1) * 2, by = (g.nv[1] != g.nv[0] ? fy : fy >> 1) * 2;
  const uint32_t *a0 = act + (int64_t)by * g.nh[0] + bx, *a1 = a0 + g.nh[0];
  iscale[fi] = (uint16_t)mask_chroma_scale(mask_scale(a0[0], A, (uint64_t)k), mask_scale(a0[1], A, (uint64_t)k),
                                           mask_scale(a1[0], A, (uint64_t)k), mask_scale(a1[1], A, (uint64_t)k));
}

inline int mask_parts(int64_t nluma) { return (int)((nluma + 255) / 256); }

// the activity of the source's luma blocks: act [nluma], part [mask_parts(nluma)]
inline hipError_t mask_launch_act(uint32_t *act, MaskPart *part, const EncPlanes &g, hipStream_t stream) {
  const int nluma = g.nh[0] * g.nv[0];
  hipLaunchKernelGGL(k_enc_mask_act, dim3((unsigned)mask_parts(nluma)), dim3(256), 0, stream, act, part, g, nluma);
  return hipGetLastError();
}

// every fragment's scale at ratio k: iscale [n], rec [1]
inline hipError_t mask_launch_scale(uint16_t *iscale, MaskRec *rec, const uint32_t *act, const MaskPart *part, const EncPlanes &g,
                                    int64_t n, int k, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_mask_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, iscale, rec, act, part,
                     mask_parts((int64_t)g.nh[0] * g.nv[0]), g, (int)n, k);
  return hipGetLastError();
}

// ---- the block-qi kernels with the scale: enc_fq_bqi with its switch on, lambda_b = (lambda iscale[fi] + 1024) >> 11 ---------------
__global__ __launch_bounds__(256) void k_enc_intra_fq_bqi_mask(int16_t *levels, int16_t *dcq, uint8_t *qii, uint32_t *overflow,
                                                               const int32_t *coded_order, EncPlanes g, const uint16_t *dequant,
                                                               const uint8_t *bqbits, BqiSel sel, const uint16_t *iscale, int64_t n) {
  EncRef R = {};
  enc_fq_bqi<0, true>(levels, dcq, qii, nullptr, nullptr, overflow, coded_order, g, R, R, (const uint32_t *)nullptr, 0, dequant,
                      bqbits, sel, n, iscale);
}

__global__ __launch_bounds__(256) void k_enc_inter_fq_bqi_mask(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap,
                                                               uint32_t *dclast, uint32_t *overflow, const int32_t *coded_order,
                                                               EncPlanes g, EncRef R, const uint32_t *mb_mode, int nmbx,
                                                               const uint16_t *dequant, const uint8_t *bqbits, BqiSel sel,
                                                               const uint16_t *iscale, int64_t n) {
  enc_fq_bqi<2, true>(levels, dcq, qii, cmap, dclast, overflow, coded_order, g, R, R, mb_mode, nmbx, dequant, bqbits, sel, n, iscale);
}

__global__ __launch_bounds__(256) void k_enc_inter_fq_all_bqi_mask(int16_t *levels, int16_t *dcq, uint8_t *qii, uint8_t *cmap,
                                                                   uint32_t *dclast, uint32_t *overflow, const int32_t *coded_order,
                                                                   EncPlanes g, EncRef R, EncRef G, const uint4 *mb_word, int nmbx,
                                                                   const uint16_t *dequant, const uint8_t *bqbits, BqiSel sel,
                                                                   const uint16_t *iscale, int64_t n) {
  enc_fq_bqi<3, true>(levels, dcq, qii, cmap, dclast, overflow, coded_order, g, R, G, mb_word, nmbx, dequant, bqbits, sel, n, iscale);
}

// ---- the launches of the quantising kernels, stated once: th_encode_* (thip_encode.hip) and thip_enc_fq_stage (theora_hip.h) both
// call these.  Each picks its kernel from sel and iscale: sel.nqis 0 the plain kernel at qi sel.q0 (qii, bqbits and iscale are not
// read), else the block-qi kernel over sel's list, with iscale (masking's scales, the map's, or both) its masked form.  dequant is the
// whole table set, of which sel names the qis: [64 qi][3][64] for a key frame, [64 qi][6][64] for an inter frame.
inline hipError_t fq_launch_key(int16_t *levels, int16_t *dcq, uint8_t *qii, uint32_t *overflow, const int32_t *order, const EncPlanes &g,
                                const uint16_t *dequant, const uint8_t *bqbits, const BqiSel &sel, const uint16_t *iscale, int64_t n,
                                hipStream_t stream) {
  const dim3 grid((unsigned)((4 * n + 255) / 256)), wg(256);
  if (!sel.nqis)
    hipLaunchKernelGGL(k_enc_intra_fq, grid, wg, 0, stream, levels, dcq, overflow, order, g, dequant + (size_t)sel.q0 * 192, n);
  else if (iscale)
    hipLaunchKernelGGL(k_enc_intra_fq_bqi_mask, grid, wg, 0, stream, levels, dcq, qii, overflow, order, g, dequant, bqbits, sel, iscale, n);
  else
    hipLaunchKernelGGL(k_enc_intra_fq_bqi, grid, wg, 0, stream, levels, dcq, qii, overflow, order, g, dequant, bqbits, sel, n);
  return hipGetLastError();
}

// Word: k_enc_me's (two reference classes, G is not read) or k_enc_me_all's (three)
template <class Word>
inline hipError_t fq_launch_inter(const InterBufs &o, uint8_t *qii, const int32_t *order, const EncPlanes &g, const EncRef &R,
                                  const EncRef &G, const Word *mb, int nmbx, const uint16_t *dequant, const uint8_t *bqbits,
                                  const BqiSel &sel, const uint16_t *iscale, int64_t n, hipStream_t stream) {
  const dim3 grid((unsigned)((4 * n + 255) / 256)), wg(256);
  if constexpr (sizeof(Word) == sizeof(uint4)) {
    if (!sel.nqis) return inter_launch_fq(o, order, g, R, G, mb, nmbx, dequant + (size_t)sel.q0 * 384, n, stream);
    if (iscale)
      hipLaunchKernelGGL(k_enc_inter_fq_all_bqi_mask, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, order, g, R,
                         G, mb, nmbx, dequant, bqbits, sel, iscale, n);
    else
      hipLaunchKernelGGL(k_enc_inter_fq_all_bqi, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, order, g, R, G, mb,
                         nmbx, dequant, bqbits, sel, n);
  } else {
    if (!sel.nqis) return inter_launch_fq(o, order, g, R, mb, nmbx, dequant + (size_t)sel.q0 * 384, n, stream);
    if (iscale)
      hipLaunchKernelGGL(k_enc_inter_fq_bqi_mask, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, order, g, R, mb,
                         nmbx, dequant, bqbits, sel, iscale, n);
    else
      hipLaunchKernelGGL(k_enc_inter_fq_bqi, grid, wg, 0, stream, o.levels, o.dcq, qii, o.cmap, o.dclast, o.overflow, order, g, R, mb, nmbx,
                         dequant, bqbits, sel, n);
  }
  return hipGetLastError();
}

}  // namespace thip
