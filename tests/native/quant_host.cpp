// Replays th_encode_*'s quantisation-parameter code (theora_amd/csrc/thip_quant.h: the check of a caller's th_quant_info, the deep
// copy, th_quant_info <-> QuantParams, the setup header's quantiser part written and parsed, the rate probe's floor) on the host,
// under AddressSanitizer and UBSan (tests/quant_host.py builds it, writes the steps and compares every printed value with
// tests/enc_quant_ref.py and the library).  No GPU, no library.
//   quant_host <steps file>
// One step a line, numbers separated by blanks:
//   set <64 dc> <64 ac> <64 limits> then for each (qti, pli): NRANGES HAVE <sizes> <(NRANGES + 1) x 64 matrix bytes>
//       (HAVE 0: NULL arrays and nothing follows; the arrays are exactly as long as NRANGES says, clamped to 0..64, so that a read
//       beyond them is the sanitizer's to find)
//   prints: set valid=0|1 and, for a valid set, nbms=N bits=<the quantiser part as '0' and '1'> again=0|1 steps_ok=0|1
//       floor=<384 numbers, commas>
//       again: the bits parsed (quant_parse), handed out (quant_info_alloc), copied (QuantCopy), consolidated and packed once more
//       are the same bits, and the copy equals the input array for array.  steps_ok: every step is in 1..32767 (rate_steps_ok's
//       range part).  floor: rate_form_floor of the steps of the parameters.
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "thip_quant.h"

using namespace thip;

namespace {

struct StrReader {   // the bit reader quant_parse asks for, over a string of '0' and '1'
  const std::string &s;
  size_t pos = 0;
  bool over = false;
  uint32_t bit() {
    if (pos >= s.size()) {
      over = true;
      return 0;
    }
    return (uint32_t)(s[pos++] - '0');
  }
  uint32_t read(int n) {
    uint32_t v = 0;
    for (int k = 0; k < n; k++) v = v << 1 | bit();
    return v;
  }
  bool overrun() const { return over; }
};

std::string pack(const QuantParams &q) {
  std::string bits;
  quant_pack(q, [&](uint32_t v, int nb) {
    for (int k = nb - 1; k >= 0; k--) bits.push_back((v >> k) & 1 ? '1' : '0');
  });
  return bits;
}

bool same_info(const th_quant_info &a, const th_quant_info &b) {
  if (memcmp(a.dc_scale, b.dc_scale, sizeof(a.dc_scale)) || memcmp(a.ac_scale, b.ac_scale, sizeof(a.ac_scale)) ||
      memcmp(a.loop_filter_limits, b.loop_filter_limits, sizeof(a.loop_filter_limits)))
    return false;
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      const th_quant_ranges &x = a.qi_ranges[qti][pli], &y = b.qi_ranges[qti][pli];
      if (x.nranges != y.nranges || memcmp(x.sizes, y.sizes, (size_t)x.nranges * sizeof(int)) ||
          memcmp(x.base_matrices, y.base_matrices, (size_t)(x.nranges + 1) * 64))
        return false;
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
    if (step != "set") return 4;
    th_quant_info qi;
    memset(&qi, 0, sizeof(qi));
    long long v;
    for (int k = 0; k < 64; k++) {
      if (!(in >> v)) return 3;
      qi.dc_scale[k] = (ogg_uint16_t)v;
    }
    for (int k = 0; k < 64; k++) {
      if (!(in >> v)) return 3;
      qi.ac_scale[k] = (ogg_uint16_t)v;
    }
    for (int k = 0; k < 64; k++) {
      if (!(in >> v)) return 3;
      qi.loop_filter_limits[k] = (unsigned char)v;
    }
    // heap arrays of exactly the stated length
    std::vector<int *> sizes;
    std::vector<unsigned char *> mats;
    for (int i = 0; i < 6; i++) {
      long long n, have;
      if (!(in >> n >> have)) return 3;
      th_quant_ranges &r = qi.qi_ranges[i / 3][i % 3];
      r.nranges = (int)n;
      if (!have) continue;
      const int len = (int)std::min<long long>(std::max<long long>(n, 0), 64);
      int *s = new int[len ? len : 1];
      unsigned char *m = new unsigned char[(size_t)(len + 1) * 64];
      sizes.push_back(s);
      mats.push_back(m);
      for (int k = 0; k < len; k++) {
        if (!(in >> v)) return 3;
        s[k] = (int)v;
      }
      for (int k = 0; k < (len + 1) * 64; k++) {
        if (!(in >> v)) return 3;
        m[k] = (unsigned char)v;
      }
      r.sizes = s;
      r.base_matrices = (const th_quant_base *)m;
    }
    const bool ok = quant_info_valid(&qi);
    printf("set valid=%d", (int)ok);
    if (ok) {
      QuantCopy copy;
      copy.assign(qi);
      QuantParams q{};
      quant_params_from_info(copy.qi, q);
      const std::string bits = pack(q);
      // parse -> hand out -> copy -> consolidate -> pack
      QuantParams parsed{};
      StrReader br{bits};
      th_quant_info out;
      bool again = quant_parse(br, parsed) == 0 && !br.overrun() && br.pos == bits.size() && quant_info_alloc(parsed, &out) == 0;
      if (again) {
        QuantCopy copy2;
        copy2.assign(out);
        quant_info_free(&out);
        QuantParams q2{};
        quant_params_from_info(copy2.qi, q2);
        QuantCopy copy3;
        copy3.assign(q2);
        again = pack(q2) == bits && same_info(copy.qi, qi) && same_info(copy2.qi, qi) && same_info(copy3.qi, qi) &&
                quant_info_valid(&copy3.qi);
      }
      std::vector<uint16_t> steps(6 * 64 * 64), floor(6 * 64);
      quant_all_steps(q, steps.data());
      rate_form_floor(floor.data(), steps.data());
      printf(" nbms=%d bits=%s again=%d steps_ok=%d floor=", q.nbms, bits.c_str(), (int)again, (int)rate_steps_ok(steps.data(), true));
      for (size_t k = 0; k < floor.size(); k++) printf("%s%u", k ? "," : "", (unsigned)floor[k]);
    }
    printf("\n");
    for (int *s : sizes) delete[] s;
    for (unsigned char *m : mats) delete[] m;
  }
  return 0;
}
