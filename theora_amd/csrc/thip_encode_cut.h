// thip_encode_cut.h -- the device side of th_encode_*'s automatic key frames (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES; the rule is stated in
// theoraenc_hip.h, "Automatic key frames").  A frame the interval rule makes an inter frame is measured before anything of it is
// queued: k_rate_me (thip_rate.h) runs the five-mode search against PREV and leaves S0, Smv, SI and the vector of every macro block,
// and the host reads back three sums of them and decides.  The search is not run again where its result is known already.
//
//   k_enc_cut_sums   k_rate_me's words reduced to P = sum min(S0, Smv), I = sum SI and N = the macro blocks with SI < min(S0, Smv):
//                    a lane a macro block, a cross-lane sum in the wave, one 64-bit atomic add a wave and sum into the 32-byte result
//                    (zeroed by a memset queued before).  Integer addition: the result does not depend on the order.
//   k_enc_mb_modes   k_enc_me's word of every macro block from k_rate_me's word and the frame's lambda (rate_mode is k_enc_me's
//                    decision): an inter frame with five modes is then coded without a second search, at any qi.
#pragma once
#include "thip_rate.h"

namespace thip {

struct CutSums {   // what the host reads back: 32 bytes
  unsigned long long pred, intra, nintra, reserved;
};

__device__ __forceinline__ uint64_t enc_sum64_wave(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
    v += (uint64_t)hi << 32 | lo;
  }
  return v;
}

// grid: ceil(nmbs / 256).  The sums are 64-bit from the lane upward: a macro block's SAD is below 2^16, so P passes 2^32 only
// beyond 65 793 macro blocks -- no picture a test can afford -- and no width is left to a size to find out.
__global__ __launch_bounds__(256) void k_enc_cut_sums(CutSums *sums, const uint4 *mbs, int nmbs) {
  const int mb = (int)(blockIdx.x * 256 + threadIdx.x);
  uint64_t p = 0, i = 0, n = 0;   // (a lane beyond nmbs adds nothing)
  if (mb < nmbs) {
    const uint4 s = mbs[mb];
    const uint32_t inter = min(s.x, s.y);
    p = inter;
    i = s.z;
    n = s.z < inter;
  }
  p = enc_sum64_wave(p);
  i = enc_sum64_wave(i);
  n = enc_sum64_wave(n);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&sums->pred, (unsigned long long)p);
    atomicAdd(&sums->intra, (unsigned long long)i);
    atomicAdd(&sums->nintra, (unsigned long long)n);
  }
}

// grid: ceil(nmbs / 256).  mb_out: k_enc_me's words (mode | mvx << 8 | mvy << 16, the vector's bytes zero unless MV)
__global__ __launch_bounds__(256) void k_enc_mb_modes(uint32_t *mb_out, const uint4 *mbs, int nmbs, int lambda) {
  const int mb = (int)(blockIdx.x * 256 + threadIdx.x);
  if (mb >= nmbs) return;
  const uint4 s = mbs[mb];
  const int mode = rate_mode(s, lambda);
  mb_out[mb] = mode == kEncPixMv ? (uint32_t)mode | (s.w & 0xFFFFu) << 8 : (uint32_t)mode;   // (s.w: mvx, mvy in its two low bytes)
}

// the launch, stated once (th_encode_* and thip_enc_inter_stage): k_enc_me's words from k_rate_me's
inline hipError_t cut_launch_mb_modes(uint32_t *mb, const uint4 *stats, int nmbs, int lambda, hipStream_t stream) {
  hipLaunchKernelGGL(k_enc_mb_modes, dim3((unsigned)((nmbs + 255) / 256)), dim3(256), 0, stream, mb, stats, nmbs, lambda);
  return hipGetLastError();
}

}  // namespace thip
