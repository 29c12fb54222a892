// Replays a scenario through th_encode_*'s rate controllers (theora_amd/csrc/thip_ratectl.h: RateCtl, TwoPass) on the host, under
// AddressSanitizer and UBSan (tests/test_encoder_rate_cpu.py and tests/test_encoder_2pass_cpu.py build it, write the scenarios and
// compare every printed field with tests/enc_rate_ref.py and tests/enc_2pass_ref.py).  No GPU, no library: the program keeps the
// frame counters th_encode_ycbcr_in and th_encode_packetout keep and calls the controllers where they do.
//   ratectl_host <scenario file>
// The scenario, one line a step, tokens separated by blanks:
//   stream fw fh pic_x pic_y pic_w pic_h fmt fps_num fps_den shift inter K   the stream (first line)
//   quality Q                  the qi of quality mode
//   bitrate B | buffer D | flags F                                           TH_ENCCTL_SET_BITRATE / _RATE_BUFFER / _RATE_FLAGS
//   frame key dups mul add E0 .. E63                                         a frame whose probe is E and whose packet takes
//                              mul x E[qi] + add bits (a record: the whole bytes of them); key: its type by the interval rule
//                              (pass 2 takes the record's); dups: the TH_ENCCTL_SET_DUP_COUNT before it
//   dup                        a duplicate packet (before the first frame: the controller's call alone, there is no packet)
//   done                       the last packet was the stream's last
//   out                        TH_ENCCTL_THIP_2PASS_OUT
//   in HEX | in -              TH_ENCCTL_THIP_2PASS_IN with these bytes (-: none)
//   want | gate                TH_ENCCTL_THIP_2PASS_IN(NULL) | may a frame come in?
// Every step prints one line: the step's name, then name=value tokens (lists joined by commas).
#include <inttypes.h>
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "thip_ratectl.h"

using namespace thip;

namespace {

EncStream st{};
RateCtl rc;
TwoPass tp;
bool rate = false, done = false;
int quality = 0;

template <class T>
void list(const char *name, const T *v, int n) {
  printf(" %s=", name);
  for (int k = 0; k < n; k++) printf("%s%" PRId64, k ? "," : "", (int64_t)v[k]);
}

void hex(const char *name, const uint8_t *p, int n) {
  printf(" %s=", name);
  for (int k = 0; k < n; k++) printf("%02x", p[k]);
  if (n <= 0) printf("-");
}

// everything the controllers hold or report after a packet
void print_packet(const char *step) {
  const thip_enc_rate_stats &r = rc.stats;
  const thip_enc_2pass_stats &t = tp.stats;
  printf("%s cur=%" PRId64 " lastkey=%" PRId64 " frame_qi=%d", step, st.cur, st.key, st.frame_qi);
  printf(" bitrate=%" PRId64 " flags=%d buf=%d started=%d T=%" PRId64 " D=%" PRId64 " R=%" PRId64 " Fstar=%" PRId64 " F=%" PRId64,
         rc.bitrate, rc.flags, rc.buf, (int)rc.started, rc.T, rc.D, rc.R, rc.Fstar, rc.F);
  list("c", rc.c, 2);
  printf(" qi=%d dropped=%d key=%d duplicate=%d target=%" PRId64 " fullness_before=%" PRId64 " fullness_after=%" PRId64
         " spend=%" PRId64 " estimate=%" PRId64 " actual=%" PRId64,
         r.qi, r.dropped, r.key, r.duplicate, r.target, r.fullness_before, r.fullness_after, r.spend, r.estimate, r.actual);
  list("probe", r.probe, 64);
  list("corr", r.corr, 2);
  printf(" tp_pass=%d tp_type=%d tp_frame=%" PRId64 " tp_qi=%d budget_left=%" PRId64 " recorded_left=%" PRId64, t.pass, t.type, t.frame,
         t.qi, t.budget_left, t.recorded_left);
  list("recorded", t.recorded, 64);
  list("fresh", t.fresh, 64);
  list("tp_corr", t.corr, 4);
  printf(" frames=%" PRId64 " dups=%" PRId64 " A=%" PRId64 "\n", tp.frames, tp.dups, tp.A);
}

// th_encode_ycbcr_in and the th_encode_packetout that follows it
void frame(bool key, int dups, int64_t mul, int64_t add, const int64_t E[64]) {
  st.dup_next = dups;
  if (tp.gate(st)) {
    printf("frame refused=%d\n", tp.gate(st));
    return;
  }
  const int64_t f = st.cur + 1;
  if (!rate) st.frame_qi = quality;
  if (tp.pass == 2) key = tp.type(st, f);
  bool dropped = false;
  if (rate || tp.pass == 1) memcpy(rc.E, E, sizeof(rc.E));
  if (rate) {
    const int qi = tp.pass == 2 ? tp.choose(st, rc, key) : rc.choose(st, key, f, key ? f : st.key);
    dropped = qi < 0;
    if (!dropped) st.frame_qi = qi;
  }
  st.dups_left = st.dup_next;
  st.dup_next = 0;
  size_t bytes = 0;
  if (dropped) {
    ++st.cur;
  } else {
    const int64_t bits = mul * E[st.frame_qi] + add;
    bytes = (size_t)(bits / 8);
    if (key) st.key = st.cur + 1;
    ++st.cur;
    if (tp.pass == 2) tp.coded(st, rc, key, bits);
    else if (rate) rc.coded(st, key, bits);
  }
  tp.packet(st, rc, dropped ? 3 : key ? 0 : 1, bytes);
  print_packet("frame");
}

void dup() {
  if (st.cur >= 0) {
    if (st.dups_left > 0) st.dups_left--;
    ++st.cur;
  }
  if (tp.pass == 2) tp.dup(st, rc);
  else if (rate) rc.dup(st);
  if (st.cur >= 0) tp.packet(st, rc, 2, 0);
  print_packet("dup");
}

void print_in(const char *step, int rc_) {
  printf("%s rc=%d tp_pass=%d stats_pass=%d hdr_ok=%d have=%zu frames=%" PRId64 " dups=%" PRId64 "\n", step, rc_, tp.pass, tp.stats.pass,
         (int)tp.hdr_ok, tp.buf.size(), tp.frames, tp.dups);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream file(argv[1]);
  std::string line;
  while (std::getline(file, line)) {
    std::istringstream in(line);
    std::string step;
    if (!(in >> step)) continue;
    if (step == "stream") {
      int inter = 0;
      in >> st.frame_width >> st.frame_height >> st.pic_x >> st.pic_y >> st.pic_width >> st.pic_height >> st.pixel_fmt >>
          st.fps_numerator >> st.fps_denominator >> st.shift >> inter >> st.kf_interval;
      st.inter = inter != 0;
      st.cur = st.key = -1;
    } else if (step == "quality") {
      in >> quality;
    } else if (step == "bitrate") {
      int64_t b = 0;
      in >> b;
      rate = true;
      rc.set_bitrate(st, b);
      print_packet("bitrate");
    } else if (step == "buffer") {
      int d = 0;
      in >> d;
      if (rc.set_buffer(st, d) != rc.buf) return 4;   // (what the request writes back is the buffer printed)
      print_packet("buffer");
    } else if (step == "flags") {
      int f = 0;
      in >> f;
      rc.set_flags(f);
      print_packet("flags");
    } else if (step == "frame") {
      int key = 0, dups = 0;
      int64_t mul = 0, add = 0, E[64];
      in >> key >> dups >> mul >> add;
      for (int q = 0; q < 64; q++) in >> E[q];
      if (!in) return 3;
      frame(key != 0, dups, mul, add, E);
    } else if (step == "dup") {
      dup();
    } else if (step == "done") {
      done = true;
    } else if (step == "out") {
      unsigned char *p = nullptr;
      const int n = tp.out(st, done, &p);
      printf("out n=%d", n);
      hex("bytes", p, n);
      printf("\n");
    } else if (step == "in") {
      std::string h;
      in >> h;
      std::vector<uint8_t> b;
      if (h != "-")
        for (size_t k = 0; k + 1 < h.size(); k += 2) b.push_back((uint8_t)std::stoi(h.substr(k, 2), nullptr, 16));
      static const uint8_t none = 0;
      print_in("in", tp.in(st, b.empty() ? &none : b.data(), b.size()));
    } else if (step == "want") {
      print_in("want", tp.in(st, nullptr, 0));
    } else if (step == "gate") {
      printf("gate rc=%d\n", tp.gate(st));
    } else {
      fprintf(stderr, "ratectl_host: unknown step %s\n", step.c_str());
      return 3;
    }
  }
  return 0;
}
