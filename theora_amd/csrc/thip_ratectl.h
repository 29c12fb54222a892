// thip_ratectl.h -- th_encode_*'s rate controllers: the one-pass controller of theoraenc_hip.h's "Bitrate mode" (RateCtl) and, of
// "Two-pass", the pass file's codec and the second controller (TwoPass).  Integer host code that includes nothing of HIP: the
// encoder (thip_encode.hip) holds one of each, gives them the probe the device measured and the packet's bits, and keeps the clock;
// tests/native/ratectl_host.cpp replays scenarios through the same code under the sanitizers.
//
// Widths.  T <= 2^40, D <= 256, a probe entry of at most 2^32 - 1, a correction <= 2^20 (Q16) and a packet of at most 2^40 bits
// keep every 64-bit intermediate below 2^63: Cur(q) <= 2^52, Future(q) <= 2^62, A << 16 <= 2^56.  The second controller's products
// are 128 bits wide and saturate at 2^62.
#ifndef THIP_RATECTL_H
#define THIP_RATECTL_H
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/theoraenc_hip.h"

namespace thip {

// what the controllers read of the stream: th_info's part of the pass file's header and the encoder's frame counters, by value
struct EncStream {
  uint32_t frame_width, frame_height, pic_x, pic_y, pic_width, pic_height, pixel_fmt, fps_numerator, fps_denominator;
  int shift;             // keyframe_granule_shift
  bool inter;
  int64_t kf_interval;
  int64_t cur, key;      // the last packet's frame and the last key frame (-1: none yet)
  int dup_next;          // the duplicates asked for the next frame
  int frame_qi;          // the last coded frame's qi
  bool frame_pending;
  int dups_left;
};

inline int64_t rate_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---- bitrate mode (theoraenc_hip.h, "Bitrate mode") ---------------------------------------------------------------------------------
struct RateCtl {
  int64_t bitrate = 0;
  int flags = TH_RATECTL_DROP_FRAMES | TH_RATECTL_CAP_OVERFLOW, buf = 0;   // buf: D when set explicitly, else 0
  bool started = false;
  int64_t T = 0, D = 0, R = 0, Fstar = 0, F = 0;
  int64_t c[2] = {65536, 65536};   // c_key, c_inter (Q16)
  int64_t L[2][64] = {};           // the last probe of each frame type
  bool L_have[2] = {false, false};
  int64_t E[64] = {};              // the probe of the frame queued
  thip_enc_rate_stats stats = {};  // (probe_ms and control_ms are the caller's)

  // T, R, F* of the bitrate in force (D kept)
  void targets(const EncStream &s) {
    T = rate_clamp((int64_t)((__int128)bitrate * s.fps_denominator / s.fps_numerator), 32, (int64_t)1 << 40);
    R = T * D;
    Fstar = R / 2;
  }

  // at the first frame
  void start(const EncStream &s) {
    if (started) return;
    D = buf ? buf : rate_clamp(s.inter ? s.kf_interval : 1, 12, 256);
    targets(s);
    F = Fstar;
    started = true;
  }

  // a new bitrate or buffer mid-stream
  void retarget(const EncStream &s) {
    if (!started) return;
    targets(s);
    F = std::min(F, R);
  }

  void set_bitrate(const EncStream &s, int64_t v) {
    bitrate = v;
    retarget(s);
  }

  // returns D as clamped
  int set_buffer(const EncStream &s, int d) {
    buf = (int)rate_clamp(d, 12, 256);
    if (started) D = buf;
    retarget(s);
    return buf;
  }

  void set_flags(int f) { flags = f & (TH_RATECTL_DROP_FRAMES | TH_RATECTL_CAP_OVERFLOW | TH_RATECTL_CAP_UNDERFLOW); }

  void caps() {
    if (flags & TH_RATECTL_CAP_OVERFLOW) F = std::min(F, R);
    if (flags & TH_RATECTL_CAP_UNDERFLOW) F = std::max(F, (int64_t)0);
  }

  // c_t after a packet of A bits coded at qi
  void correct(bool key, int qi, int64_t A) {
    const int t = key ? 0 : 1;
    c[t] = rate_clamp((c[t] + (A << 16) / std::max(E[qi], (int64_t)1)) / 2, 4096, (int64_t)1 << 20);
  }

  // the statistics of a choice, and of what the packet left behind
  void chosen(int qi, bool drop, bool key, int64_t before, int64_t spend, int64_t estimate) {
    stats.qi = qi;
    stats.dropped = drop;
    stats.key = key && !drop;
    stats.duplicate = 0;
    stats.target = T;
    stats.fullness_before = before;
    stats.spend = spend;
    stats.estimate = estimate;
    stats.actual = 0;
    memcpy(stats.probe, E, sizeof(stats.probe));
  }
  void after(int64_t fullness) {
    stats.fullness_after = fullness;
    stats.corr[0] = c[0];
    stats.corr[1] = c[1];
  }

  // the choice for frame f, probed into E; keypos: the key position the interval rule counts from.  Returns the qi, or -1 to drop
  int choose(const EncStream &s, bool key, int64_t f, int64_t keypos) {
    start(s);
    const int t = key ? 0 : 1;
    memcpy(L[t], E, sizeof(E));
    L_have[t] = true;
    // the next D - 1 frames: key or inter by the interval rule from the current key position
    int64_t nk = 0, ni = 0;
    for (int64_t m = f + 1; m < f + D; m++) {
      if (!s.inter || (m - keypos) % s.kf_interval == 0) nk++;
      else ni++;
    }
    int64_t cur[64], fut[64];
    for (int q = 0; q < 64; q++) {
      cur[q] = E[q] * c[t] >> 16;
      int64_t kt = L_have[0] ? L[0][q] * c[0] >> 16 : -1;
      int64_t it = L_have[1] ? L[1][q] * c[1] >> 16 : -1;
      if (it < 0) it = kt / 4;
      if (kt < 0) kt = 4 * it;
      fut[q] = nk * kt + ni * it;
    }
    const int64_t S = F + D * T - Fstar;
    int qi = 0;
    for (int q = 63; q >= 0; q--)
      if (cur[q] + fut[q] <= S) {
        qi = q;
        break;
      }
    const int64_t full = (int64_t)1 << s.shift;
    const bool drop = (flags & TH_RATECTL_DROP_FRAMES) && s.cur >= 0 && F + T - cur[0] < 0 && s.key >= 0 && f - s.key + s.dup_next < full;
    chosen(drop ? s.frame_qi : qi, drop, key, F, S, cur[qi]);
    if (drop) {
      F += T;
      caps();
    }
    after(F);
    return drop ? -1 : qi;
  }

  // after a frame coded at s.frame_qi in A bits
  void coded(const EncStream &s, bool key, int64_t A) {
    F += T - A;
    caps();
    correct(key, s.frame_qi, A);
    stats.actual = A;
    after(F);
  }

  // a duplicate (TH_ENCCTL_SET_DUP_COUNT); false before the first frame, when it is nothing
  bool dup(const EncStream &s) {
    if (!started) return false;
    stats.dropped = stats.key = 0;
    stats.duplicate = 1;
    stats.qi = s.frame_qi;
    stats.fullness_before = F;
    F += T;
    caps();
    stats.fullness_after = F;
    stats.spend = stats.estimate = stats.actual = 0;
    memset(stats.probe, 0, sizeof(stats.probe));
    stats.probe_ms = stats.control_ms = 0;
    return true;
  }
};

// ---- two-pass (theoraenc_hip.h, "Two-pass") -----------------------------------------------------------------------------------------
// pass 1 writes the pass file; pass 2 reads it and chooses with the RateCtl's T, c and E (the controller's buffer is not used)
struct TwoPass {
  int pass = 0;                          // 0, 1 (out), 2 (in)
  bool rec_ready = false, final_out = false;
  int64_t frames = 0, dups = 0;          // pass 1: the counts so far; pass 2: the header's
  uint64_t tot[2][64] = {};              // pass 1: the sums so far; pass 2: the header's
  uint64_t seen[2][64] = {}, fresh[2][64] = {};   // pass 2: per class, the recorded and the fresh curves of the frames so far
  int64_t A = 0, ratio[2] = {65536, 65536};
  int cls = -1;                          // pass 2: the class of the record the frame queued follows (-1: none)
  int64_t rec[64] = {};                  // ... and its curve
  bool hdr_ok = false;
  std::vector<uint8_t> buf;              // pass 1: what the last out() returned; pass 2: the pass file so far
  uint8_t record[THIP_2PASS_RECORD_BYTES] = {};
  thip_enc_2pass_stats stats = {};       // (wait_ms is the caller's)

  static void put(uint8_t *p, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; k++) p[k] = (uint8_t)(v >> (8 * k));
  }
  static uint64_t get(const uint8_t *p, int bytes) {
    uint64_t v = 0;
    for (int k = 0; k < bytes; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
  }

  // the eleven u32 of the header that must be the stream's
  static void fields(const EncStream &s, uint32_t f[11]) {
    const uint32_t v[11] = {s.frame_width, s.frame_height, s.pic_x, s.pic_y, s.pic_width, s.pic_height, s.pixel_fmt,
                            s.fps_numerator, s.fps_denominator, (uint32_t)s.shift, s.inter ? 1u : 0u};
    memcpy(f, v, sizeof(v));
  }

  // a record's class: the sum its curve enters (-1: none)
  static int class_of(const EncStream &s, int type) { return type <= 1 ? type : type == 3 ? (s.inter ? 1 : 0) : -1; }

  // B - A: what the budget leaves
  int64_t left(const RateCtl &rc) const { return rc.T * (frames + dups) - A; }

  // pass 1: the header of the pass file with the counts and sums so far (all 0 for the placeholder) into buf
  void header(const EncStream &s) {
    buf.assign(THIP_2PASS_HEADER_BYTES, 0);
    uint8_t *p = buf.data();
    memcpy(p, "THP2", 4);
    put(p + 4, 1, 4);
    uint32_t f[11];
    fields(s, f);
    for (int k = 0; k < 11; k++) put(p + 8 + 4 * k, f[k], 4);
    put(p + 52, (uint64_t)frames, 4);
    put(p + 56, (uint64_t)dups, 4);
    for (int t = 0; t < 2; t++)
      for (int q = 0; q < 64; q++) put(p + 60 + 8 * (t * 64 + q), tot[t][q], 8);
  }

  // TH_ENCCTL_THIP_2PASS_OUT (never in pass 2; in pass 0 before the first frame only): the placeholder, the last packet's record,
  // the finished header once the stream is done, then nothing
  int out(const EncStream &s, bool done, unsigned char **p) {
    if (pass == 0) {
      pass = stats.pass = 1;
    } else if (rec_ready) {
      rec_ready = false;
      *p = record;
      return THIP_2PASS_RECORD_BYTES;
    } else if (done && !final_out) {
      final_out = true;
    } else {
      *p = nullptr;
      return 0;
    }
    header(s);
    *p = buf.data();
    return THIP_2PASS_HEADER_BYTES;
  }

  // every packet of `bytes` bytes: the statistics of the pass, and in pass 1 the packet's record.  type: 0 key, 1 inter,
  // 2 duplicate, 3 dropped
  void packet(const EncStream &s, const RateCtl &rc, int type, size_t bytes) {
    stats.pass = pass;
    stats.frame = s.cur;
    stats.qi = s.frame_qi;
    if (pass == 0) return;
    const bool probed = type != 2;
    stats.probe_ms = probed ? rc.stats.probe_ms : 0.0;
    for (int q = 0; q < 64; q++) stats.fresh[q] = probed ? rc.E[q] : 0;
    if (pass == 2) {
      stats.type = type == 2 ? 2 : stats.type;   // (a frame: the record's type, set when the frame was queued)
      if (type == 2) memset(stats.recorded, 0, sizeof(stats.recorded));
      stats.budget_left = left(rc);
      stats.corr[0] = rc.c[0];
      stats.corr[1] = rc.c[1];
      stats.corr[2] = ratio[0];
      stats.corr[3] = ratio[1];
      return;
    }
    stats.type = type;
    uint8_t *p = record;
    memset(p, 0, sizeof(record));
    p[0] = (uint8_t)type;
    p[1] = (uint8_t)s.frame_qi;
    put(p + 4, std::min<uint64_t>((uint64_t)bytes * 8, 0xFFFFFFFFu), 4);
    const int k = class_of(s, type);
    for (int q = 0; q < 64; q++) {
      const uint64_t v = probed ? (uint64_t)std::min<int64_t>(std::max<int64_t>(rc.E[q], 0), 0xFFFFFFFFll) : 0;
      put(p + 8 + 4 * q, v, 4);
      stats.recorded[q] = (int64_t)v;
      if (k >= 0) tot[k][q] += v;
    }
    if (type == 2) dups++;
    else frames++;
    rec_ready = true;
  }

  // pass 2: the bytes still wanted before frame n can be taken (n: the next frame's index)
  int64_t wanted(const EncStream &s) const {
    const int64_t have = (int64_t)buf.size();
    if (!hdr_ok) return THIP_2PASS_HEADER_BYTES - have;
    const int64_t n = s.cur + 1 + (s.frame_pending ? 1 : 0) + s.dups_left;
    if (n >= frames + dups) return 0;
    return std::max<int64_t>(THIP_2PASS_HEADER_BYTES + (n + 1) * THIP_2PASS_RECORD_BYTES - have, 0);
  }

  // TH_ENCCTL_THIP_2PASS_IN (never in pass 1; in pass 0 in bitrate mode before the first frame only): bytes of the pass file, and
  // how many were consumed; p = NULL: how many are wanted
  int in(const EncStream &s, const uint8_t *p, size_t n) {
    pass = stats.pass = 2;
    if (!p) return (int)std::min<int64_t>(wanted(s), 0x7FFFFFFF);
    n = std::min(n, (size_t)0x7FFFFFFF);
    size_t used = 0;
    int bad = 0;
    if (!hdr_ok) {
      used = std::min(n, (size_t)THIP_2PASS_HEADER_BYTES - buf.size());
      buf.insert(buf.end(), p, p + used);
      const uint8_t *h = buf.data();
      if (buf.size() >= 8 && (memcmp(h, "THP2", 4) != 0 || get(h + 4, 4) != 1)) bad = TH_ENOTFORMAT;
      if (!bad && buf.size() == THIP_2PASS_HEADER_BYTES) {
        uint32_t f[11];
        fields(s, f);
        for (int k = 0; k < 11; k++)
          if (get(h + 8 + 4 * k, 4) != f[k]) bad = TH_EINVAL;
        if (!bad) {
          frames = (int64_t)get(h + 52, 4);
          dups = (int64_t)get(h + 56, 4);
          for (int t = 0; t < 2; t++)
            for (int q = 0; q < 64; q++) tot[t][q] = get(h + 60 + 8 * (t * 64 + q), 8);
          hdr_ok = true;
        }
      }
      if (bad) {   // as before the pass file's first byte
        buf.clear();
        pass = stats.pass = 0;
        return bad;
      }
      if (!hdr_ok) return (int)used;
    }
    const size_t total = (size_t)THIP_2PASS_HEADER_BYTES + (size_t)(frames + dups) * THIP_2PASS_RECORD_BYTES;
    const size_t take = std::min(n - used, total - buf.size());
    buf.insert(buf.end(), p + used, p + used + take);
    return (int)(used + take);
  }

  // pass 2: may the next frame be taken?
  int gate(const EncStream &s) const {
    if (pass != 2) return 0;
    if (!hdr_ok || s.cur + 1 >= frames + dups || wanted(s) > 0) return TH_EINVAL;
    return 0;
  }

  // pass 2: is frame f a key frame?  By its record; the record's curve enters Seen
  bool type(const EncStream &s, int64_t f) {
    const uint8_t *r = buf.data() + THIP_2PASS_HEADER_BYTES + (size_t)f * THIP_2PASS_RECORD_BYTES;
    const int type = r[0] <= 3 ? r[0] : 1;
    const int64_t full = (int64_t)1 << s.shift;
    cls = class_of(s, type);
    stats.type = type;
    for (int q = 0; q < 64; q++) {
      rec[q] = (int64_t)get(r + 8 + 4 * q, 4);
      stats.recorded[q] = rec[q];
      if (cls >= 0) seen[cls][q] += (uint64_t)rec[q];
    }
    return type == 0 || !s.inter || s.key < 0 || f - s.key + s.dup_next >= full;
  }

  // pass 2: Y_u(q), what the recorded curves leave of class u at q, scaled by fresh / recorded of the frames so far and by c_u
  __int128 rest(const RateCtl &rc, int u, int q) const {
    if (tot[u][q] <= seen[u][q]) return 0;
    unsigned __int128 y = tot[u][q] - seen[u][q];
    if (seen[u][q]) y = std::min<unsigned __int128>(y * fresh[u][q] / seen[u][q], (unsigned __int128)1 << 62);
    return (__int128)y * rc.c[u] >> 16;
  }

  // pass 2: the choice for the frame probed into rc.E
  int choose(const EncStream &s, RateCtl &rc, bool key) {
    rc.start(s);
    const int t = key ? 0 : 1;
    if (cls >= 0)
      for (int q = 0; q < 64; q++)
        fresh[cls][q] = std::min<uint64_t>(fresh[cls][q] + (uint64_t)std::max<int64_t>(rc.E[q], 0), 1ull << 62);
    const int64_t budget = left(rc);
    int qi = 0;
    int64_t est = 0;
    for (int q = 63; q >= 0; q--) {
      const int64_t cur = rc.E[q] * rc.c[t] >> 16;
      const __int128 fut = rest(rc, 0, q) + rest(rc, 1, q);
      if (q == 0) est = cur;
      if ((__int128)cur + fut <= budget) {
        qi = q;
        est = cur;
        break;
      }
    }
    int64_t rl = 0;
    for (int u = 0; u < 2; u++) {
      if (tot[u][qi] > seen[u][qi]) rl += (int64_t)(tot[u][qi] - seen[u][qi]);
      ratio[u] = seen[u][qi] ? (int64_t)std::min<unsigned __int128>(((unsigned __int128)fresh[u][qi] << 16) / seen[u][qi],
                                                                    (unsigned __int128)1 << 62)
                             : 65536;
    }
    stats.recorded_left = rl;
    rc.chosen(qi, false, key, budget, budget, est);
    rc.after(budget);
    return qi;
  }

  // pass 2: after a frame coded at s.frame_qi in A bits
  void coded(const EncStream &s, RateCtl &rc, bool key, int64_t bits) {
    A += bits;
    rc.correct(key, s.frame_qi, bits);
    rc.stats.actual = bits;
    rc.after(left(rc));
  }

  // pass 2: a duplicate (no buffer: B - A before and after)
  void dup(const EncStream &s, RateCtl &rc) {
    if (rc.dup(s)) rc.stats.fullness_before = rc.stats.fullness_after = left(rc);
  }
};

}  // namespace thip
#endif
