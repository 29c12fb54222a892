// thip_quant.h -- th_encode_*'s quantisation parameters as data (theoraenc_hip.h, "Quantisation parameters"): the check of a
// caller's th_quant_info, its deep copy, the parser of the setup header's quantiser part, th_quant_info <-> QuantParams (thip_bitstream.h: what compute_qmat and the setup header's
// parser work with), the quantiser part of the setup header as libtheora's oc_quant_params_pack writes it, and the rate probe's floor
// (thip_rate.h).  Host code that includes nothing of HIP: thip_encode.hip answers TH_ENCCTL_SET_QUANT_PARAMS and writes its setup
// header through it, thip_frontend.cpp answers thip_quant_info_from_setup through it; tests/native/quant_host.cpp replays the same
// code under the sanitizers.
#ifndef THIP_QUANT_H
#define THIP_QUANT_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/theoraenc_hip.h"
#include "thip_bitstream.h"

namespace thip {

// A parameter set is valid when every (qti, pli) has 1..63 ranges, arrays that are there, sizes >= 1 that sum to exactly 63, and
// no loop-filter limit is above 127 (the header's 3 bits of nbits carry at most 7 bits a limit).  Everything else is legal, as it
// is to the decoder: any scale, any base-matrix byte (qmin of spec 6.4.3 bounds every step from below).
inline bool quant_info_valid(const th_quant_info *qi) {
  if (!qi) return false;
  for (int q = 0; q < 64; q++)
    if (qi->loop_filter_limits[q] > 127) return false;
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      const th_quant_ranges &r = qi->qi_ranges[qti][pli];
      if (r.nranges < 1 || r.nranges > 63 || !r.sizes || !r.base_matrices) return false;
      int sum = 0;
      for (int k = 0; k < r.nranges; k++) {
        if (r.sizes[k] < 1 || r.sizes[k] > 63) return false;
        sum += r.sizes[k];
      }
      if (sum != 63) return false;
    }
  return true;
}

// A th_quant_info that owns what its pointers point to (the context's copy: TH_ENCCTL_THIP_GET_QUANT_PARAMS hands `qi` out)
struct QuantCopy {
  th_quant_info qi;
  std::vector<int> sizes[2][3];
  std::vector<unsigned char> mats[2][3];   // (nranges + 1) x 64
  QuantCopy() { memset(&qi, 0, sizeof(qi)); }
  QuantCopy(const QuantCopy &) = delete;
  QuantCopy &operator=(const QuantCopy &) = delete;
  void point() {
    for (int qti = 0; qti < 2; qti++)
      for (int pli = 0; pli < 3; pli++) {
        qi.qi_ranges[qti][pli].nranges = (int)sizes[qti][pli].size();
        qi.qi_ranges[qti][pli].sizes = sizes[qti][pli].data();
        qi.qi_ranges[qti][pli].base_matrices = (const th_quant_base *)mats[qti][pli].data();
      }
  }
  void assign(const th_quant_info &src) {   // a VALID set
    memcpy(qi.dc_scale, src.dc_scale, sizeof(qi.dc_scale));
    memcpy(qi.ac_scale, src.ac_scale, sizeof(qi.ac_scale));
    memcpy(qi.loop_filter_limits, src.loop_filter_limits, sizeof(qi.loop_filter_limits));
    for (int qti = 0; qti < 2; qti++)
      for (int pli = 0; pli < 3; pli++) {
        const th_quant_ranges &r = src.qi_ranges[qti][pli];
        sizes[qti][pli].assign(r.sizes, r.sizes + r.nranges);
        const unsigned char *m = &r.base_matrices[0][0];
        mats[qti][pli].assign(m, m + (size_t)(r.nranges + 1) * 64);
      }
    point();
  }
  void assign(const QuantParams &q) {   // the stream's parameters, each (qti, pli) with matrices of its own
    for (int k = 0; k < 64; k++) {
      qi.dc_scale[k] = q.dcscale[k];
      qi.ac_scale[k] = q.acscale[k];
      qi.loop_filter_limits[k] = q.lflims[k];
    }
    for (int qti = 0; qti < 2; qti++)
      for (int pli = 0; pli < 3; pli++) {
        const int n = q.nqrs[qti][pli];
        sizes[qti][pli].assign(q.qrsizes[qti][pli], q.qrsizes[qti][pli] + n);
        mats[qti][pli].resize((size_t)(n + 1) * 64);
        for (int k = 0; k <= n; k++) memcpy(&mats[qti][pli][(size_t)k * 64], &q.bms[(size_t)q.qrbmis[qti][pli][k] * 64], 64);
      }
    point();
  }
};

// QuantParams of a valid th_quant_info.  The base matrices are consolidated by content, in first-seen order over (qti, pli, range
// end): the list and the indices the setup header carries (at most 6 x 64 = 384 matrices, what its 9 bits hold).
inline void quant_params_from_info(const th_quant_info &qi, QuantParams &q) {
  for (int k = 0; k < 64; k++) {
    q.dcscale[k] = qi.dc_scale[k];
    q.acscale[k] = qi.ac_scale[k];
    q.lflims[k] = qi.loop_filter_limits[k];
  }
  q.nbms = 0;
  q.bms.clear();
  memset(q.qrsizes, 0, sizeof(q.qrsizes));
  memset(q.qrbmis, 0, sizeof(q.qrbmis));
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      const th_quant_ranges &r = qi.qi_ranges[qti][pli];
      q.nqrs[qti][pli] = r.nranges;
      for (int k = 0; k < r.nranges; k++) q.qrsizes[qti][pli][k] = r.sizes[k];
      for (int k = 0; k <= r.nranges; k++) {
        int b = 0;
        while (b < q.nbms && memcmp(&q.bms[(size_t)b * 64], r.base_matrices[k], 64) != 0) b++;
        if (b == q.nbms) {
          q.bms.insert(q.bms.end(), r.base_matrices[k], r.base_matrices[k] + 64);
          q.nbms++;
        }
        q.qrbmis[qti][pli][k] = b;
      }
    }
}

// The quantiser part of the setup header (spec 6.4.1 - 6.4.2) from consolidated parameters, as libtheora's oc_quant_params_pack
// writes it: limits and scales with the bit widths of the largest value; each (qti, pli) after the first writes "01" when qti > 0
// and its ranges (count, sizes, indices) equal those of (qti - 1, pli), else "0" (qti = 0) or "00" (qti > 0) when they equal those
// of the previous (qti, pli) in the order of the six, else a 1 and its ranges.  put(value, nbits), MSB first.
template <class Put>
inline void quant_pack(const QuantParams &q, Put put) {
  int nb = 0;
  for (int k = 0; k < 64; k++) nb = std::max(nb, ilog(q.lflims[k]));
  put((uint32_t)nb, 3);
  for (int k = 0; k < 64; k++) put(q.lflims[k], nb);
  for (const uint16_t *sc : {q.acscale, q.dcscale}) {
    nb = 1;
    for (int k = 0; k < 64; k++) nb = std::max(nb, ilog(sc[k]));
    put((uint32_t)nb - 1, 4);
    for (int k = 0; k < 64; k++) put(sc[k], nb);
  }
  put((uint32_t)q.nbms - 1, 9);
  for (size_t k = 0; k < (size_t)q.nbms * 64; k++) put(q.bms[k], 8);
  const int bmbits = ilog((uint32_t)q.nbms - 1);
  auto same = [&](int a, int b) {   // the ranges of (qti, pli) number a and b of the six
    const int n = q.nqrs[a / 3][a % 3];
    return n == q.nqrs[b / 3][b % 3] && memcmp(q.qrsizes[a / 3][a % 3], q.qrsizes[b / 3][b % 3], (size_t)n * sizeof(int)) == 0 &&
           memcmp(q.qrbmis[a / 3][a % 3], q.qrbmis[b / 3][b % 3], (size_t)(n + 1) * sizeof(int)) == 0;
  };
  for (int i = 0; i < 6; i++) {
    const int qti = i / 3, pli = i % 3;
    if (i > 0) {
      if (qti > 0 && same(i, i - 3)) {
        put(1, 2);
        continue;
      }
      if (same(i, i - 1)) {
        put(0, qti > 0 ? 2 : 1);
        continue;
      }
      put(1, 1);
    }
    put((uint32_t)q.qrbmis[qti][pli][0], bmbits);
    for (int qri = 0, qi = 0; qri < q.nqrs[qti][pli]; qri++) {
      put((uint32_t)q.qrsizes[qti][pli][qri] - 1, ilog((uint32_t)(62 - qi)));
      qi += q.qrsizes[qti][pli][qri];
      put((uint32_t)q.qrbmis[qti][pli][qri + 1], bmbits);
    }
  }
}

// The quantiser part of a setup header (spec 6.4.1 - 6.4.2) into q: the one parser, which th_decode_headerin's parse_setup
// (thip_frontend.cpp) calls with its bit reader.  br: read(nbits), bit(), overrun().  0, or TH_EBADHEADER
template <class Reader>
inline int quant_parse(Reader &br, QuantParams &q) {
  int nbits = (int)br.read(3);   // 6.4.1 loop filter limits
  for (int qi = 0; qi < 64; qi++) q.lflims[qi] = (uint8_t)br.read(nbits);
  nbits = (int)br.read(4) + 1;   // 6.4.2 quantization parameters
  for (int qi = 0; qi < 64; qi++) q.acscale[qi] = (uint16_t)br.read(nbits);
  nbits = (int)br.read(4) + 1;
  for (int qi = 0; qi < 64; qi++) q.dcscale[qi] = (uint16_t)br.read(nbits);
  q.nbms = (int)br.read(9) + 1;
  if (q.nbms > 384 || br.overrun()) return TH_EBADHEADER;
  q.bms.resize((size_t)q.nbms * 64);
  for (int i = 0; i < q.nbms * 64; i++) q.bms[i] = (uint8_t)br.read(8);
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      int newqr = 1;
      if (qti > 0 || pli > 0) newqr = (int)br.bit();
      if (!newqr) {
        int rpqr = 0;
        if (qti > 0) rpqr = (int)br.bit();
        int qtj, plj;
        if (rpqr) {
          qtj = qti - 1;
          plj = pli;
        } else {
          qtj = (3 * qti + pli - 1) / 3;
          plj = (pli + 2) % 3;
        }
        q.nqrs[qti][pli] = q.nqrs[qtj][plj];
        memcpy(q.qrsizes[qti][pli], q.qrsizes[qtj][plj], sizeof(q.qrsizes[0][0]));
        memcpy(q.qrbmis[qti][pli], q.qrbmis[qtj][plj], sizeof(q.qrbmis[0][0]));
      } else {
        int qri = 0, qi = 0;
        q.qrbmis[qti][pli][0] = (int)br.read(ilog((uint32_t)q.nbms - 1));
        if (q.qrbmis[qti][pli][0] >= q.nbms) return TH_EBADHEADER;
        do {
          q.qrsizes[qti][pli][qri] = (int)br.read(ilog((uint32_t)(62 - qi))) + 1;
          qi += q.qrsizes[qti][pli][qri];
          qri++;
          q.qrbmis[qti][pli][qri] = (int)br.read(ilog((uint32_t)q.nbms - 1));
          if (q.qrbmis[qti][pli][qri] >= q.nbms) return TH_EBADHEADER;
        } while (qi < 63 && qri < 63);
        if (qi != 63) return TH_EBADHEADER;
        q.nqrs[qti][pli] = qri;
      }
    }
  return 0;
}

// thip_quant_info_from_setup's result: arrays of malloc, one pair a (qti, pli), freed by quant_info_free.  TH_EFAULT: no memory
inline void quant_info_free(th_quant_info *qi) {
  if (!qi) return;
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      free(const_cast<int *>(qi->qi_ranges[qti][pli].sizes));
      free(const_cast<th_quant_base *>(qi->qi_ranges[qti][pli].base_matrices));
    }
  memset(qi, 0, sizeof(*qi));
}
inline int quant_info_alloc(const QuantParams &q, th_quant_info *out) {
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < 64; k++) {
    out->dc_scale[k] = q.dcscale[k];
    out->ac_scale[k] = q.acscale[k];
    out->loop_filter_limits[k] = q.lflims[k];
  }
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      const int n = q.nqrs[qti][pli];
      int *sizes = (int *)malloc((size_t)n * sizeof(int));
      th_quant_base *mats = (th_quant_base *)malloc((size_t)(n + 1) * sizeof(th_quant_base));
      out->qi_ranges[qti][pli].nranges = n;
      out->qi_ranges[qti][pli].sizes = sizes;
      out->qi_ranges[qti][pli].base_matrices = mats;
      if (!sizes || !mats) {
        quant_info_free(out);
        return TH_EFAULT;
      }
      for (int k = 0; k < n; k++) sizes[k] = q.qrsizes[qti][pli][k];
      for (int k = 0; k <= n; k++) memcpy(mats[k], &q.bms[(size_t)q.qrbmis[qti][pli][k] * 64], 64);
    }
  return 0;
}

// every step of the parameters: [6 tables][64 q][64 z], the intra then the inter table of each plane, zig-zag order
inline void quant_all_steps(const QuantParams &q, uint16_t *steps) {
  for (int t = 0; t < 6; t++)
    for (int qi = 0; qi < 64; qi++) compute_qmat(q, t / 3, t % 3, qi, &steps[(t * 64 + qi) * 64]);
}

// the rate probe's floor (thip_rate.h): the least step over q of each (table, z), from the steps [6][64 q][64 z].  k_rate_dc and
// k_rate_tok walk the indices whose coefficient is not zero under the floor, a superset of those not zero at any q, whatever the
// order of the steps in q.  (With steps that fall with q, the built-in ones, the floor is column 63.)
inline void rate_form_floor(uint16_t *floor, const uint16_t *steps) {
  for (int t = 0; t < 6; t++)
    for (int z = 0; z < 64; z++) {
      uint16_t m = steps[(t * 64 + 0) * 64 + z];
      for (int q = 1; q < 64; q++) m = std::min(m, steps[(t * 64 + q) * 64 + z]);
      floor[t * 64 + z] = m;
    }
}

// what the probe asks of a table set: every step in 1..32767.  any_order = false asks, besides, that the step of every (table, z)
// at qi 63 be the least over q: what the kernels once rested on (they balloted at qi 63) and thip_enc_rate_stage still asks of a
// caller who has not set thip_enc_rate_req.any_order.  th_encode_* does not ask it: the kernels ballot against the floor.
inline bool rate_steps_ok(const uint16_t *steps, bool any_order = false) {
  for (int t = 0; t < 6; t++)
    for (int q = 0; q < 64; q++)
      for (int z = 0; z < 64; z++) {
        const int d = steps[(t * 64 + q) * 64 + z];
        if (d < 1 || d > 32767 || (!any_order && d < steps[(t * 64 + 63) * 64 + z])) return false;
      }
  return true;
}

}  // namespace thip
#endif
