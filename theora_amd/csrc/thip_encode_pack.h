// thip_encode_pack.h -- the device packetiser of th_encode_* (TH_ENCCTL_THIP_SET_DEVICE_PACK): what the host packer of
// thip_encode.hip does with the frame's tokens -- EOB runs merged, the four Huffman tables chosen, the bits written -- on the device,
// bit for bit.  In: the token words k_enc_intra_scatter leaves in stream order (thip_encode.h) and the 3 x 64 list lengths.  That
// buffer is the same for key and inter frames, five or eight modes, block-level qi and bitrate mode: one code path for all.
//
// The stream of T tokens is cut into gridDim.x contiguous spans (a multiple of 256 tokens each), one work group a span, the same cut
// in every kernel.  Five launches, none of which waits for another work group (every cross-group quantity is written by one launch
// and read by a later one):
//
//   k_enc_pack_edges   per span: the index after its last token that is not an EOB (0: none).  Zeroes the histogram.
//   k_enc_pack_merge   the EOB runs.  The run an EOB at index i belongs to starts at m(i) = the largest such index at or before i --
//                      an inclusive max-scan, carried into the span from k_enc_pack_edges' words of the spans before it.  A run is
//                      cut into pieces of 4095 from its start; the LAST word of a piece (position 4094 in it, or the stream's next
//                      word is no EOB) emits the piece's token, so only the distance to the run's start is needed, and the piece's
//                      list (index, plane) is read from its first word, (i - position).  Emitting at the last word instead of the
//                      first leaves the order of the merged tokens as it is: the words between emit nothing.  Out: one merged word
//                      a stream word (0: emits nothing) and the histogram [5 groups][luma, chroma][32 tokens].
//   k_enc_pack_bits    every work group chooses the four tables from the histogram (64 threads: choice x table; 64-bit sums; a tie
//                      goes to the lower index) and sums its span's bits, merged tokens and merged AC tokens.
//   k_enc_pack_scan    one work group: the exclusive scan of the spans' sums, and the record the host reads.
//   k_enc_pack_place   after the host knows the header's length: each tile of 256 tokens builds its bits in LDS (a token is at most
//                      32 + 12 bits, 8 more with the AC table indices in front of it: at most three 32-bit words), stores the
//                      interior words plainly and ORs its first and last word, which a neighbouring tile may share, into memory the
//                      host's memset zeroed.  Words are MSB first; the bytes are swapped when a word is stored.
//
// Bit positions: the token bits start at bit `phase` (the header's length mod 8) of byte 0.  The DC table indices (8 bits) come first;
// a merged token whose list index is 0 stands at phase + 8 + (bits of the tokens before it), one of a higher index 8 bits further,
// and the first such token carries the AC table indices in front of it (with none, the last tile puts them at the end).  Stream
// order is by index first, so every index-0 token precedes every other.  Bit totals are 64-bit; inside a tile 16 bits suffice
// (256 x 44 < 65536).
#pragma once
#include "thip_bitstream.h"
#include "thip_encode.h"

namespace thip {

constexpr int kPackMaxGroups = 512;
constexpr uint32_t kPackEmit = 1u << 21;   // merged word: token | extra << 5 (12 bits) | chroma << 17 | Huffman group << 18 | emit
// a tile's bits: 7 + 8 + 256 x 44 + 8 + 8, and the word alignment at both ends.  44 is the conservative bound -- a code of 32 bits and
// the 12 extra bits of the long EOB run in every lane, where a tile holds at most 8 such runs (32 EOBs each).  What tables of 32-bit
// codes reach, and tests/test_gpu_pack_direct.py drives, is 256 x 42 (the value token of 10 extra bits) + 8 + 8 + 7 + 31 = 10 806
// bits, 338 words.  A caller's code set (TH_ENCCTL_SET_HUFFMAN_CODES) may put a 31-bit code on the long EOB run: 43 bits a token, 51
// with the AC table indices in front, which tests/test_gpu_encoder_huff.py drives through a packet and through one tile.
constexpr int kPackBufWords = 368;

struct PackSum {   // a span's sums, or (after the scan) those of all spans before it
  unsigned long long bits;
  uint32_t cnt, ac;
};
struct PackRec {   // what the host reads
  unsigned long long bits;   // of the merged tokens (the 16 bits of table indices not counted)
  uint32_t merged, nac;      // merged tokens; those of a list index above 0
  int32_t hti[4];            // DC luma, DC chroma, AC luma, AC chroma
  uint32_t total, pad;       // tokens before the merge
};

// T, and the calling work group's span [a, b) of it
__device__ __forceinline__ uint32_t pack_span(const uint32_t *list_len, uint32_t *s_w, uint32_t &a, uint32_t &b) {
  uint32_t excl;
  const uint32_t T = enc_block_scan(threadIdx.x < 192 ? list_len[threadIdx.x] : 0u, excl, s_w);
  const uint32_t S = ((T + gridDim.x - 1) / gridDim.x + 255u) & ~255u;
  const unsigned long long a0 = (unsigned long long)blockIdx.x * S;
  a = (uint32_t)min(a0, (unsigned long long)T);
  b = (uint32_t)min(a0 + S, (unsigned long long)T);
  return T;
}

__global__ __launch_bounds__(256) void k_enc_pack_edges(uint32_t *glast, uint32_t *hist, const uint32_t *out, const uint32_t *list_len) {
  __shared__ uint32_t s_w[4], s_max;
  uint32_t a, b;
  pack_span(list_len, s_w, a, b);
  if (blockIdx.x == 0)
    for (int k = (int)threadIdx.x; k < 320; k += 256) hist[k] = 0;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t i = a + threadIdx.x; i < b; i += 256)
    if (out[i] & 31u) m = i + 1;
  if (m) atomicMax(&s_max, m);
  __syncthreads();
  if (threadIdx.x == 0) glast[blockIdx.x] = s_max;
}

// inclusive prefix maximum over the 256 threads of a work group (s_w: 4 words of LDS); all: the maximum of all
__device__ __forceinline__ uint32_t pack_block_maxscan(uint32_t v, uint32_t &all, uint32_t *s_w) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x = max(x, y);
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  uint32_t before = 0;
  all = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t c = s_w[q];
    before = max(before, q < w ? c : 0u);
    all = max(all, c);
  }
  __syncthreads();
  return max(before, x);
}

__device__ __forceinline__ int pack_huff_group(int z) { return z == 0 ? 0 : z <= 5 ? 1 : z <= 14 ? 2 : z <= 27 ? 3 : 4; }

// mtok [T], hist [5][2][32] (zeroed by k_enc_pack_edges), glast: k_enc_pack_edges'
__global__ __launch_bounds__(256) void k_enc_pack_merge(uint32_t *mtok, uint32_t *hist, const uint32_t *glast, const uint32_t *out,
                                                        const uint32_t *list_len) {
  __shared__ uint32_t s_w[4], s_hist[320], s_c;
  uint32_t a, b;
  const uint32_t T = pack_span(list_len, s_w, a, b);
  for (int k = (int)threadIdx.x; k < 320; k += 256) s_hist[k] = 0;
  if (threadIdx.x == 0) s_c = 0;
  __syncthreads();
  uint32_t c = 0;   // the index after the last token before the span that is no EOB
  for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256) c = max(c, glast[j]);
  if (c) atomicMax(&s_c, c);
  __syncthreads();
  c = s_c;
  for (uint32_t t0 = a; t0 < b; t0 += 256) {
    const uint32_t i = t0 + threadIdx.x;
    const bool in = i < b;
    const uint32_t w = in ? out[i] : 1u;
    const bool eob = (w & 31u) == 0;
    uint32_t all;
    const uint32_t m = max(c, pack_block_maxscan(eob ? 0u : i + 1, all, s_w));
    c = max(c, all);
    if (!in) continue;   // (after the tile's barriers)
    uint32_t mw = 0, lw = w, te = w & 0xFFFFu;
    bool emit = !eob;
    if (eob) {
      const uint32_t pos = (i - m) % 4095u;   // in its piece
      emit = pos == 4094u || i + 1 >= T || (out[i + 1] & 31u) != 0;
      if (emit) {
        const uint32_t run = pos + 1;
        lw = out[i - pos];   // the piece's first word: its list
        te = run <= 3 ? run - 1 : run <= 7 ? 3u | (run - 4) << 5 : run <= 15 ? 4u | (run - 8) << 5 : run <= 31 ? 5u | (run - 16) << 5
                                                                                                               : 6u | run << 5;
      }
    }
    if (emit) {
      const uint32_t hg = (uint32_t)pack_huff_group((int)(lw >> 16) & 63), ch = (lw >> 22) != 0;
      mw = te | ch << 17 | hg << 18 | kPackEmit;
      atomicAdd(&s_hist[(hg * 2 + ch) * 32 + (te & 31u)], 1u);
    }
    mtok[i] = mw;
  }
  __syncthreads();
  for (int k = (int)threadIdx.x; k < 320; k += 256)
    if (s_hist[k]) atomicAdd(&hist[k], s_hist[k]);
}

// the four tables of least bits (s_hist: the histogram in LDS; cl [80][32]: code length | extra bits << 8); ends with a barrier
__device__ __forceinline__ void pack_choose_tables(int *s_hti, unsigned long long *s_cost, const uint32_t *s_hist, const uint32_t *cl) {
  if (threadIdx.x < 64) {
    const int c = (int)threadIdx.x >> 4, t = (int)threadIdx.x & 15, ac = c >> 1, ch = c & 1;
    unsigned long long bits = 0;
    for (int hg = ac ? 1 : 0; hg < (ac ? 5 : 1); hg++)
      for (int tok = 0; tok < 32; tok++)
        bits += (unsigned long long)s_hist[(hg * 2 + ch) * 32 + tok] * (cl[(16 * hg + t) * 32 + tok] & 0xFFu);
    s_cost[threadIdx.x] = bits;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int best = 0;
    for (int t = 1; t < 16; t++)
      if (s_cost[threadIdx.x * 16 + t] < s_cost[threadIdx.x * 16 + best]) best = t;
    s_hti[threadIdx.x] = best;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_enc_pack_bits(PackSum *gsum, PackRec *rec, const uint32_t *mtok, const uint32_t *hist,
                                                       const uint32_t *cl, const uint32_t *list_len) {
  __shared__ uint32_t s_w[4], s_hist[320], s_bits[320], s_cnt, s_ac;
  __shared__ int s_hti[4];
  __shared__ unsigned long long s_cost[64], s_sum;
  uint32_t a, b;
  const uint32_t T = pack_span(list_len, s_w, a, b);
  for (int k = (int)threadIdx.x; k < 320; k += 256) s_hist[k] = hist[k];
  if (threadIdx.x == 0) {
    s_sum = 0;
    s_cnt = s_ac = 0;
  }
  __syncthreads();
  pack_choose_tables(s_hti, s_cost, s_hist, cl);
  for (int k = (int)threadIdx.x; k < 320; k += 256) {
    const int hg = k >> 6;
    const uint32_t e = cl[(16 * hg + s_hti[(hg ? 2 : 0) + ((k >> 5) & 1)]) * 32 + (k & 31)];
    s_bits[k] = (e & 0xFFu) + (e >> 8);
  }
  __syncthreads();
  unsigned long long bits = 0;
  uint32_t cnt = 0, ac = 0;
  for (uint32_t i = a + threadIdx.x; i < b; i += 256) {
    const uint32_t mw = mtok[i];
    if (mw & kPackEmit) {
      bits += s_bits[((mw >> 17) & 15u) * 32 + (mw & 31u)];
      cnt++;
      ac += (mw >> 18 & 7u) != 0;
    }
  }
  if (cnt) {
    atomicAdd(&s_sum, bits);
    atomicAdd(&s_cnt, cnt);
    atomicAdd(&s_ac, ac);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    gsum[blockIdx.x] = PackSum{s_sum, s_cnt, s_ac};
    if (blockIdx.x == 0) {
      for (int c = 0; c < 4; c++) rec->hti[c] = s_hti[c];
      rec->total = T;
      rec->pad = 0;
    }
  }
}

// enc_block_scan on 64-bit values
__device__ __forceinline__ unsigned long long pack_block_scan64(unsigned long long v, unsigned long long &excl, unsigned long long *s_w) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  unsigned long long x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  unsigned long long before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const unsigned long long c = s_w[q];
    before += q < w ? c : 0ull;
    total += c;
  }
  __syncthreads();
  excl = before + x - v;
  return total;
}

// one work group: gbase [ngroups] = the sums of the spans before each; rec: the totals
__global__ __launch_bounds__(256) void k_enc_pack_scan(PackSum *gbase, PackRec *rec, const PackSum *gsum, int ngroups) {
  __shared__ uint32_t s_w[4];
  __shared__ unsigned long long s_w64[4];
  unsigned long long rbits = 0;
  uint32_t rcnt = 0, rac = 0;
  for (int g0 = 0; g0 < ngroups; g0 += 256) {
    const int g = g0 + (int)threadIdx.x;
    const PackSum v = g < ngroups ? gsum[g] : PackSum{0, 0, 0};
    unsigned long long eb;
    uint32_t ec, ea;
    const unsigned long long tb = pack_block_scan64(v.bits, eb, s_w64);
    const uint32_t tc = enc_block_scan(v.cnt, ec, s_w), ta = enc_block_scan(v.ac, ea, s_w);
    if (g < ngroups) gbase[g] = PackSum{rbits + eb, rcnt + ec, rac + ea};
    rbits += tb;
    rcnt += tc;
    rac += ta;
  }
  if (threadIdx.x == 0) {
    rec->bits = rbits;
    rec->merged = rcnt;
    rec->nac = rac;
  }
}

// nb bits of val (1..52), MSB first, at bit r of the tile's words
__device__ __forceinline__ void pack_put(uint32_t *buf, unsigned long long val, int nb, uint32_t r) {
  const unsigned long long V = val << (64 - nb);
  const int s = (int)(r & 31u);
  const uint32_t k = r >> 5;
  const unsigned long long X = V >> s;
  const uint32_t w0 = (uint32_t)(X >> 32), w1 = (uint32_t)X, w2 = s ? (uint32_t)((V << (64 - s)) >> 32) : 0u;
  if (w0) atomicOr(&buf[k], w0);
  if (w1) atomicOr(&buf[k + 1], w1);
  if (w2) atomicOr(&buf[k + 2], w2);
}

// pk [cap_words], zeroed over the packet's bytes; codes [80][32]; phase 0..7
__global__ __launch_bounds__(256) void k_enc_pack_place(uint32_t *pk, uint32_t cap_words, const PackSum *gbase, const PackRec *rec,
                                                        const uint32_t *mtok, const uint32_t *codes, const uint32_t *cl,
                                                        const uint32_t *list_len, int phase) {
  __shared__ uint32_t s_w[4], s_code[320], s_cl[320], s_buf[kPackBufWords];
  uint32_t a, b;
  pack_span(list_len, s_w, a, b);
  int hti[4];
#pragma unroll
  for (int c = 0; c < 4; c++) hti[c] = rec->hti[c];
  for (int k = (int)threadIdx.x; k < 320; k += 256) {
    const int hg = k >> 6, h = (16 * hg + hti[(hg ? 2 : 0) + ((k >> 5) & 1)]) * 32 + (k & 31);
    s_code[k] = codes[h];
    s_cl[k] = cl[h];
  }
  __syncthreads();
  const unsigned long long total = rec->bits;
  const PackSum base = gbase[blockIdx.x];
  unsigned long long run = base.bits;
  uint32_t acb = base.ac;
  const bool g_first = blockIdx.x == 0, g_last = blockIdx.x == gridDim.x - 1;
  uint32_t ntiles = (b - a + 255u) / 256u;
  // the table indices in front and, with no AC token, at the end, also where the span is empty.  (With no token of a class every
  // table ties at 0 bits and the indices are 0, which the memset wrote: in an empty span this states where they go and changes
  // no byte.)
  if ((g_first || g_last) && !ntiles) ntiles = 1;
  const uint32_t hdr_dc = (uint32_t)(hti[0] << 4 | hti[1]), hdr_ac = (uint32_t)(hti[2] << 4 | hti[3]);
  for (uint32_t t = 0; t < ntiles; t++) {
    const uint32_t i = a + t * 256u + threadIdx.x;
    const uint32_t mw = i < b ? mtok[i] : 0u;
    const bool emit = (mw & kPackEmit) != 0;
    unsigned long long val = 0;
    int nb = 0;
    uint32_t ac = 0;
    if (emit) {
      const uint32_t k = ((mw >> 17) & 15u) * 32 + (mw & 31u), e = s_cl[k], xb = e >> 8;
      val = (unsigned long long)s_code[k] << xb | ((mw >> 5) & ((1u << xb) - 1u));
      nb = (int)((e & 0xFFu) + xb);
      ac = (mw >> 18 & 7u) != 0;
    }
    uint32_t excl;
    const uint32_t tot = enc_block_scan((uint32_t)nb | ac << 16, excl, s_w);
    const uint32_t tbits = tot & 0xFFFFu, tac = tot >> 16, ebits = excl & 0xFFFFu, eac = excl >> 16;
    const bool first = g_first && t == 0, last = g_last && t == ntiles - 1;
    const unsigned long long tlo = first ? 0ull : (unsigned long long)phase + 8 + run + (acb ? 8 : 0);
    const unsigned long long thi = last ? (unsigned long long)phase + 16 + total
                                        : (unsigned long long)phase + 8 + run + tbits + (acb + tac ? 8 : 0);
    if (thi > tlo) {   // (the same for the whole work group)
      const unsigned long long wlo = tlo >> 5;
      const uint32_t nw = (uint32_t)(((thi - 1) >> 5) - wlo) + 1;
      for (uint32_t k = threadIdx.x; k < (uint32_t)kPackBufWords; k += 256) s_buf[k] = 0;
      __syncthreads();
      if (emit) {
        unsigned long long pos = (unsigned long long)phase + 8 + run + ebits + (ac ? 8 : 0);
        if (ac && acb + eac == 0) {   // the first token of an index above 0: the AC table indices stand in front of it
          val |= (unsigned long long)hdr_ac << nb;
          nb += 8;
          pos -= 8;
        }
        pack_put(s_buf, val, nb, (uint32_t)(pos - wlo * 32));
      }
      if (threadIdx.x == 0 && first) pack_put(s_buf, hdr_dc, 8, (uint32_t)phase);
      if (threadIdx.x == 0 && last && acb + tac == 0) pack_put(s_buf, hdr_ac, 8, (uint32_t)((unsigned long long)phase + 8 + total - wlo * 32));
      __syncthreads();
      for (uint32_t k = threadIdx.x; k < nw; k += 256) {
        const uint32_t w = __builtin_bswap32(s_buf[k]);
        const unsigned long long at = wlo + k;
        if (at >= cap_words) continue;
        if (k == 0 || k == nw - 1) {   // a neighbouring tile may hold the word's other bits
          if (w) atomicOr(&pk[at], w);
        } else {
          pk[at] = w;
        }
      }
      __syncthreads();
    }
    run += tbits;
    acb += tac;
  }
}

// ---- the launches, stated once: th_encode_* (thip_encode.hip) and thip_enc_pack_tokens (theora_hip.h) both call these -----------
struct PackBufs {                  // device memory of one packetiser
  uint32_t *glast, *hist;          // [groups], [320]
  uint32_t *codes, *cl;            // [80][32]: the codes; code length | extra bits << 8 (pack_cl_table)
  uint32_t *mtok;                  // [T]: the merged words
  PackSum *gsum, *gbase;           // [groups]
  PackRec *rec;
};

inline void pack_cl_table(uint32_t cl[80 * 32], const uint8_t len[80][32]) {
  for (int h = 0; h < 80; h++)
    for (int tok = 0; tok < 32; tok++) cl[h * 32 + tok] = (uint32_t)len[h][tok] | (uint32_t)kTokExtraBits[tok] << 8;
}

// everything that does not need the phase: the merge, the tables, the sums and their scan.  words: the token words in stream order;
// list_len: 192 words whose sum is T; groups: 1..kPackMaxGroups.  p.rec holds the record when the stream gets there.
inline hipError_t pack_launch_sums(const PackBufs &p, const uint32_t *words, const uint32_t *list_len, int groups, hipStream_t stream) {
  const dim3 grid((unsigned)groups), wg(256);
  hipError_t rc;
  hipLaunchKernelGGL(k_enc_pack_edges, grid, wg, 0, stream, p.glast, p.hist, words, list_len);
  if ((rc = hipGetLastError()) != hipSuccess) return rc;
  hipLaunchKernelGGL(k_enc_pack_merge, grid, wg, 0, stream, p.mtok, p.hist, (const uint32_t *)p.glast, words, list_len);
  if ((rc = hipGetLastError()) != hipSuccess) return rc;
  hipLaunchKernelGGL(k_enc_pack_bits, grid, wg, 0, stream, p.gsum, p.rec, (const uint32_t *)p.mtok, (const uint32_t *)p.hist,
                     (const uint32_t *)p.cl, list_len);
  if ((rc = hipGetLastError()) != hipSuccess) return rc;
  hipLaunchKernelGGL(k_enc_pack_scan, dim3(1), wg, 0, stream, p.gbase, p.rec, (const PackSum *)p.gsum, groups);
  return hipGetLastError();
}

// the bytes the token bits take from bit `phase` of byte 0, given the record's bits; and whether they fit a buffer of `cap` bytes
// (pack_launch_place zeroes whole words)
inline uint64_t pack_need_bytes(int phase, uint64_t bits) { return ((uint64_t)phase + 16 + bits + 7) >> 3; }
inline bool pack_fits(uint64_t need, uint64_t cap) { return need + 4 <= cap; }

// the bits, after pack_launch_sums on the same stream with the same list_len and groups: pk (4-byte aligned, pack_fits(need, its
// size)) is zeroed over the packet's words and written; nothing at or beyond byte 4 * ceil(need / 4) is touched
inline hipError_t pack_launch_place(const PackBufs &p, const uint32_t *list_len, int groups, int phase, uint8_t *pk, uint64_t need,
                                    hipStream_t stream) {
  const size_t nwords = (size_t)((need + 3) >> 2);
  const hipError_t rc = hipMemsetAsync(pk, 0, nwords * 4, stream);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(k_enc_pack_place, dim3((unsigned)groups), dim3(256), 0, stream, (uint32_t *)pk, (uint32_t)nwords,
                     (const PackSum *)p.gbase, (const PackRec *)p.rec, (const uint32_t *)p.mtok, (const uint32_t *)p.codes,
                     (const uint32_t *)p.cl, list_len, phase);
  return hipGetLastError();
}

}  // namespace thip
