// Replays th_encode_*'s Huffman-code arithmetic (theora_amd/csrc/thip_hufftrain.h: the check of a code set, the setup header's trees
// from the codes, the trainer) on the host, under AddressSanitizer and UBSan (tests/hufftrain_host.py builds it, writes the steps and
// compares every printed value with tests/enc_huff_ref.py).  No GPU, no library.
//   hufftrain_host <steps file>
// One step a line, numbers separated by blanks; a code set is 2560 pairs "pattern nbits", set by set, token by token:
//   valid <code set>                              prints: valid ok=0|1
//   trees <code set>                              prints: trees nbits=N bits=<the 80 trees as '0' and '1'>   (a valid set)
//   train ROUNDS N <start code set> <N x 320 counts: group, class, token>
//                                                 prints: train rc=.. bits_start=.. bits_end=.. rounds=.. dc_tables=.. ac_tables=..
//                                                         samples=.. codes=<2560 pairs joined by commas>
#include <inttypes.h>
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "thip_hufftrain.h"

using namespace thip;

namespace {

bool read_codes(std::istringstream &in, std::vector<th_huff_code> &c) {
  c.resize(80 * 32);
  for (auto &e : c) {
    long long pat, nb;
    if (!(in >> pat >> nb)) return false;
    e.pattern = (uint32_t)pat;
    e.nbits = (int)nb;
  }
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string step;
    if (!(in >> step)) continue;
    std::vector<th_huff_code> codes;
    if (step == "valid") {
      if (!read_codes(in, codes)) return 3;
      printf("valid ok=%d\n", (int)huff_codes_valid((const th_huff_code(*)[32])codes.data()));
    } else if (step == "trees") {
      if (!read_codes(in, codes)) return 3;
      std::string bits;
      for (int h = 0; h < 80; h++)
        huff_tree_write(&codes[h * 32], [&](uint32_t v, int nb) {
          for (int k = nb - 1; k >= 0; k--) bits.push_back((v >> k) & 1 ? '1' : '0');
        });
      printf("trees nbits=%zu bits=%s\n", bits.size(), bits.c_str());
    } else if (step == "train") {
      int rounds;
      size_t n;
      if (!(in >> rounds >> n) || !read_codes(in, codes)) return 3;
      std::vector<thip_enc_token_hist> hists(n);
      for (auto &h : hists) {
        memset(&h, 0, sizeof(h));
        for (int g = 0; g < 5; g++)
          for (int c = 0; c < 2; c++)
            for (int t = 0; t < 32; t++) {
              unsigned long long v;
              if (!(in >> v)) return 3;
              h.count[g][c][t] = (uint32_t)v;
            }
      }
      std::vector<th_huff_code> out(80 * 32);
      thip_huff_train_stats st;
      memset(&st, 0, sizeof(st));
      const int rc = huff_train(n ? hists.data() : nullptr, n, (const th_huff_code(*)[32])codes.data(), rounds,
                                (th_huff_code(*)[32])out.data(), &st);
      printf("train rc=%d bits_start=%" PRIu64 " bits_end=%" PRIu64 " rounds=%d dc_tables=%d ac_tables=%d samples=%d codes=", rc,
             st.bits_start, st.bits_end, st.rounds, st.dc_tables, st.ac_tables, st.samples);
      for (size_t k = 0; k < out.size(); k++) printf("%s%u,%d", k ? "," : "", rc ? 0u : out[k].pattern, rc ? 0 : out[k].nbits);
      printf("\n");
    } else {
      return 4;
    }
  }
  return 0;
}
