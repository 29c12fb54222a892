// thip_hufftrain.h -- th_encode_*'s Huffman codes as data (theoraenc_hip.h, "Huffman codes"): the Huffman code of 32 integer
// weights (the rule of the built-in trees), the check of a caller's code set, the setup header's trees from the codes, and the
// trainer thip_huff_train.  Integer host code that includes nothing of HIP: thip_encode.hip builds its setup with it and answers
// TH_ENCCTL_SET_HUFFMAN_CODES through it; tests/native/hufftrain_host.cpp replays the same code under the sanitizers.
//
// Widths.  Every sum is an unsigned 64-bit integer and wraps: a histogram sum H, a node weight 1024 H + 1 and its sums over a
// tree, a cost sum of count x length.  They are exact while the counts of all histograms together stay below 2^49.
#ifndef THIP_HUFFTRAIN_H
#define THIP_HUFFTRAIN_H
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/theoraenc_hip.h"

namespace thip {

// Huffman code of 32 weights: always merge the two lightest (ties: the lower node id; leaves are 0..31, internal nodes are numbered
// from 32 in creation order); child 0 = the lighter.  No code is longer than 31 bits.
inline void huff_build(const uint64_t w[32], uint32_t code[32], uint8_t len[32]) {
  struct Node { uint64_t w; int c0, c1; };
  Node nodes[63];
  int live[32], nlive = 32, nnodes = 32;
  for (int k = 0; k < 32; k++) {
    nodes[k] = Node{w[k], -1, -1};
    live[k] = k;   // (ascending ids, and a new node has the highest: it stays so)
  }
  auto lighter = [&](int x, int y) { return nodes[x].w < nodes[y].w || (nodes[x].w == nodes[y].w && x < y); };
  while (nlive > 1) {
    int ia = 0;
    for (int i = 1; i < nlive; i++)
      if (lighter(live[i], live[ia])) ia = i;
    int ib = ia ? 0 : 1;
    for (int i = 0; i < nlive; i++)
      if (i != ia && lighter(live[i], live[ib])) ib = i;
    const int a = live[ia], b = live[ib];
    nodes[nnodes] = Node{nodes[a].w + nodes[b].w, a, b};
    int n = 0;
    for (int i = 0; i < nlive; i++)
      if (i != ia && i != ib) live[n++] = live[i];
    live[n++] = nnodes++;
    nlive = n;
  }
  // the codes, root first: a node's children are made before it, so a descending pass sees every parent before its children
  uint32_t c[63];
  uint8_t l[63];
  c[nnodes - 1] = 0;
  l[nnodes - 1] = 0;
  for (int x = nnodes - 1; x >= 32; x--) {
    c[nodes[x].c0] = c[x] << 1;
    c[nodes[x].c1] = c[x] << 1 | 1;
    l[nodes[x].c0] = l[nodes[x].c1] = (uint8_t)(l[x] + 1);
  }
  for (int k = 0; k < 32; k++) {
    code[k] = c[k];
    len[k] = l[k];
  }
}

// one set of 32 codes: every token has a code of 1..32 bits and the codes form a full, prefix-free binary code (what the
// reference's oc_huff_codes_pack accepts); bits of a pattern above nbits are ignored.  order: the tokens by rising code, which is
// the order of the tree's leaves
inline bool huff_set_valid(const th_huff_code c[32], int order[32]) {
  uint64_t start[32];
  for (int k = 0; k < 32; k++) {
    if (c[k].nbits < 1 || c[k].nbits > 32) return false;
    const uint64_t pat = (uint64_t)c[k].pattern & (((uint64_t)1 << c[k].nbits) - 1);
    start[k] = pat << (32 - c[k].nbits);   // the code's interval of 32-bit strings starts here ...
    order[k] = k;
  }
  std::sort(order, order + 32, [&](int x, int y) { return start[x] < start[y] || (start[x] == start[y] && x < y); });
  uint64_t at = 0;
  for (int j = 0; j < 32; j++) {   // ... and the intervals tile [0, 2^32) exactly
    const int k = order[j];
    if (start[k] != at) return false;
    at += (uint64_t)1 << (32 - c[k].nbits);
  }
  return at == (uint64_t)1 << 32;
}

inline bool huff_codes_valid(const th_huff_code codes[80][32]) {
  int order[32];
  for (int h = 0; h < 80; h++)
    if (!huff_set_valid(codes[h], order)) return false;
  return true;
}

// the tree of one valid set as the setup header states it (spec 6.4.4): pre-order, the 0 branch first; 0 = an internal node,
// 1 and five bits of token = a leaf.  put(value, bits) takes them
template <class Put>
inline void huff_tree_write(const th_huff_code c[32], Put put) {
  int order[32];
  if (!huff_set_valid(c, order)) return;
  int d = -1;   // the depth of the node whose 1 branch the next leaf lies under
  for (int j = 0; j < 32; j++) {
    const th_huff_code &e = c[order[j]];
    for (int k = d + 1; k < e.nbits; k++) put(0u, 1);
    put(1u, 1);
    put((uint32_t)order[j], 5);
    uint32_t p = e.pattern;
    d = e.nbits;
    while (d > 0 && (p & 1)) {
      p >>= 1;
      d--;
    }
    d--;
  }
}

// ---- the trainer (theoraenc_hip.h, "Huffman codes") -------------------------------------------------------------------------------
struct HuffTrainer {
  struct Sample { uint32_t packet; uint8_t cls, ac; };   // count[0][cls] (DC) or count[1..4][cls] (AC) of hists[packet]
  const thip_enc_token_hist *hists;
  std::vector<Sample> samples;
  std::vector<uint8_t> assign, trial;

  // the table of least cost for every sample (ties: the lower index) -> the total cost
  uint64_t assign_all(const th_huff_code codes[80][32], std::vector<uint8_t> &a) const {
    uint64_t total = 0;
    a.resize(samples.size());
    for (size_t s = 0; s < samples.size(); s++) {
      const Sample &x = samples[s];
      const thip_enc_token_hist &h = hists[x.packet];
      uint64_t best = 0;
      int bt = 0;
      for (int t = 0; t < 16; t++) {
        uint64_t bits = 0;
        for (int hg = x.ac ? 1 : 0; hg < (x.ac ? 5 : 1); hg++)
          for (int tok = 0; tok < 32; tok++) bits += (uint64_t)h.count[hg][x.cls][tok] * (uint64_t)codes[16 * hg + t][tok].nbits;
        if (t == 0 || bits < best) {
          best = bits;
          bt = t;
        }
      }
      a[s] = (uint8_t)bt;
      total += best;
    }
    return total;
  }

  // every table with a sample, rebuilt from its samples' counts
  void rebuild(th_huff_code codes[80][32]) const {
    for (int ac = 0; ac < 2; ac++)
      for (int t = 0; t < 16; t++)
        for (int hg = ac ? 1 : 0; hg < (ac ? 5 : 1); hg++) {
          uint64_t w[32] = {};
          bool any = false;
          for (size_t s = 0; s < samples.size(); s++) {
            const Sample &x = samples[s];
            if (x.ac != ac || assign[s] != t) continue;
            any = true;
            for (int tok = 0; tok < 32; tok++) w[tok] += hists[x.packet].count[hg][x.cls][tok];
          }
          if (!any) continue;
          for (int tok = 0; tok < 32; tok++) w[tok] = 1024 * w[tok] + 1;
          uint32_t code[32];
          uint8_t len[32];
          huff_build(w, code, len);
          for (int tok = 0; tok < 32; tok++) codes[16 * hg + t][tok] = th_huff_code{code[tok], (int)len[tok]};
        }
  }
};

// thip_huff_train with `start` never NULL (the caller passes the built-in codes for NULL)
inline int huff_train(const thip_enc_token_hist *hists, size_t n, const th_huff_code start[80][32], int rounds,
                      th_huff_code out[80][32], thip_huff_train_stats *stats) {
  if (!start || !out || (n && !hists)) return TH_EFAULT;
  if (n > ((size_t)1 << 20) || rounds < 1 || rounds > 64 || !huff_codes_valid(start)) return TH_EINVAL;
  HuffTrainer T;
  T.hists = hists;
  for (size_t p = 0; p < n; p++)
    for (int cls = 0; cls < 2; cls++)
      for (int ac = 0; ac < 2; ac++) {
        bool any = false;
        for (int hg = ac ? 1 : 0; hg < (ac ? 5 : 1); hg++)
          for (int tok = 0; tok < 32; tok++) any |= hists[p].count[hg][cls][tok] != 0;
        if (any) T.samples.push_back(HuffTrainer::Sample{(uint32_t)p, (uint8_t)cls, (uint8_t)ac});
      }
  std::vector<th_huff_code> cur(80 * 32), next(80 * 32);
  auto tab = [](std::vector<th_huff_code> &v) { return (th_huff_code(*)[32])v.data(); };
  for (int h = 0; h < 80; h++)
    for (int tok = 0; tok < 32; tok++) {
      const th_huff_code &c = start[h][tok];
      cur[h * 32 + tok] = th_huff_code{(uint32_t)((uint64_t)c.pattern & (((uint64_t)1 << c.nbits) - 1)), c.nbits};
    }
  uint64_t B = T.assign_all(tab(cur), T.assign);
  const uint64_t B0 = B;
  int accepted = 0;
  for (int r = 0; r < rounds; r++) {
    next = cur;
    T.rebuild(tab(next));
    const uint64_t B1 = T.assign_all(tab(next), T.trial);
    if (B1 >= B) break;
    cur.swap(next);
    T.assign.swap(T.trial);
    B = B1;
    accepted++;
  }
  memcpy(out, cur.data(), sizeof(th_huff_code) * 80 * 32);
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->bits_start = B0;
    stats->bits_end = B;
    stats->rounds = accepted;
    stats->samples = (int32_t)T.samples.size();
    uint32_t used[2] = {0, 0};
    for (size_t s = 0; s < T.samples.size(); s++) used[T.samples[s].ac] |= 1u << T.assign[s];
    stats->dc_tables = __builtin_popcount(used[0]);
    stats->ac_tables = __builtin_popcount(used[1]);
  }
  return 0;
}

}  // namespace thip
#endif
