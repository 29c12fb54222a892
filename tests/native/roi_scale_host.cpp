// k_enc_roi_scale's lane (roi_lane of theora_amd/csrc/thip_encode_roi.h) built for the host, fragment by fragment, under
// AddressSanitizer and UBSan (tests/test_encoder_roi_cpu.py compiles and runs this): every byte round the map's rows -- the padding
// between them included -- and round the output is poisoned, so a load that is not an entry of the map or a store outside the output
// stops the program; every scale is compared with a plain restatement of include/theoraenc_hip.h's rule, sample by sample.
#include <sanitizer/asan_interface.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "thip_encode_roi.h"   // (-I theora_amd/csrc)

using namespace thip;

struct Map {   // hm rows of wm bytes at pitch (negative: row 0 last in memory), row 0 `off` past a 4-byte boundary; the rest poisoned
  std::vector<uint8_t> mem;
  int8_t *row0;
  int wm, hm;
  int64_t pitch;
  Map(int wm_, int hm_, int64_t pitch_, int off) : wm(wm_), hm(hm_), pitch(pitch_) {
    const int64_t ap = pitch < 0 ? -pitch : pitch;
    mem.resize(64 + 8 + (size_t)hm * ap + 64, 0x55);
    uint8_t *lo = (uint8_t *)((((uintptr_t)mem.data() + 32 + 3) & ~(uintptr_t)3) + off);
    row0 = (int8_t *)(pitch < 0 ? lo + (int64_t)(hm - 1) * ap : lo);
    ASAN_POISON_MEMORY_REGION(mem.data(), mem.size());
    for (int y = 0; y < hm; y++) {
      ASAN_UNPOISON_MEMORY_REGION(row0 + y * pitch, wm);
      for (int x = 0; x < wm; x++) row0[y * pitch + x] = (int8_t)(rand() % 129 - 64);
    }
  }
  ~Map() { ASAN_UNPOISON_MEMORY_REGION(mem.data(), mem.size()); }
  int at(int x, int y) const { return row0[y * pitch + x]; }
};

static const int kT[16] = THIP_ROI_T;

// the rule, sample by sample, in 64-bit integers
static uint32_t want(const Map &m, const RoiGeo &q, uint32_t mask, int p, int fx, int fy, int &e) {
  const int hd = p ? q.hdec : 0, vd = p ? q.vdec : 0;
  int64_t S = 0;
  for (int r = 0; r < 8; r++)
    for (int c = 0; c < 8; c++) {
      int64_t x = ((int64_t)(fx * 8 + c) << hd) - q.px0, y = ((int64_t)((q.nv[p] - 1 - fy) * 8 + r) << vd) - q.py0;
      x = x < 0 ? 0 : x > q.pw - 1 ? q.pw - 1 : x;
      y = y < 0 ? 0 : y > q.ph - 1 ? q.ph - 1 : y;
      S += m.at((int)(x * q.wm / q.pw), (int)(y * q.hm / q.ph));
    }
  e = (int)((S + 32) >> 6);
  const int n = -e, o = n >> 4, f = n & 15;
  const int64_t r = o >= 0 ? (int64_t)kT[f] << o : ((int64_t)kT[f] + ((int64_t)1 << (-o - 1))) >> -o;
  const int64_t i = ((int64_t)mask * r + 1024) >> 11;
  return (uint32_t)(i < 128 ? 128 : i > 32768 ? 32768 : i);
}

static long run(int fw, int fh, int fmt, int px, int py, int pw, int ph, int wm, int hm, int pad, int off, bool neg, bool masked) {
  RoiGeo q;
  q.hdec = !(fmt & 1);
  q.vdec = !(fmt & 2);
  int n = 0;
  for (int p = 0; p < 3; p++) {
    q.nh[p] = (fw >> 3) >> (p ? q.hdec : 0);
    q.nv[p] = (fh >> 3) >> (p ? q.vdec : 0);
    q.froff[p] = n;
    n += q.nh[p] * q.nv[p];
  }
  q.px0 = px, q.py0 = py, q.pw = pw, q.ph = ph, q.wm = wm, q.hm = hm, q.nfrags = n;
  q.pitch = neg ? -(int64_t)(wm + pad) : wm + pad;
  Map m(wm, hm, q.pitch, off);
  const bool dwords = (((uintptr_t)m.row0 | (uintptr_t)q.pitch) & 3) == 0;
  // the output between poisoned guards; masking's scales likewise
  std::vector<uint16_t> out((size_t)n + 64, 0), mask((size_t)n + 64, 0);
  for (int k = 0; k < n; k++) mask[32 + k] = (uint16_t)(128 + rand() % (32768 - 128 + 1));
  ASAN_POISON_MEMORY_REGION(out.data(), 64);
  ASAN_POISON_MEMORY_REGION(out.data() + 32 + n, 64);
  ASAN_POISON_MEMORY_REGION(mask.data(), 64);
  ASAN_POISON_MEMORY_REGION(mask.data() + 32 + n, 64);
  for (int wide = 0; wide < 2; wide++)
    for (int fi = 0; fi < n; fi++) {
      int p, e, we;
      const uint16_t *mk = masked ? mask.data() + 32 : nullptr;
      const uint32_t got = wide ? roi_lane<true>(m.row0, mk, q, dwords, fi, p, e) : roi_lane<false>(m.row0, mk, q, dwords, fi, p, e);
      out[32 + fi] = (uint16_t)got;
      const int loc = fi - q.froff[p];
      const uint32_t w = want(m, q, masked ? mask[32 + fi] : 2048u, p, loc % q.nh[p], loc / q.nh[p], we);
      if (got != w || e != we || out[32 + fi] != w) {
        printf("mismatch frame %dx%d fmt %d pic %d,%d %dx%d map %dx%d pad %d off %d neg %d masked %d wide %d fragment %d: %u (e %d), want %u (e %d)\n",
               fw, fh, fmt, px, py, pw, ph, wm, hm, pad, off, (int)neg, (int)masked, wide, fi, got, e, w, we);
        exit(1);
      }
    }
  ASAN_UNPOISON_MEMORY_REGION(out.data(), out.size() * 2);
  ASAN_UNPOISON_MEMORY_REGION(mask.data(), mask.size() * 2);
  return 2L * n;
}

int main() {
  long cases = 0, lanes = 0;
  // the exponent's ends and the table, by themselves
  for (int e = -64; e <= 64; e++)
    if (roi_scale(e) < 128u || roi_scale(e) > 32768u || (e == 0 && roi_scale(e) != 2048u)) return printf("roi_scale(%d) = %u\n", e, roi_scale(e)), 1;
  if (roi_final(128, 128) != 128u || roi_final(32768, 32768) != 32768u || roi_final(2048, 2048) != 2048u) return printf("roi_final\n"), 1;
  struct G { int fw, fh, px, py, pw, ph; };
  const G geos[] = {{64, 48, 0, 0, 64, 48}, {80, 64, 5, 3, 67, 49}, {32, 16, 0, 0, 32, 16}};
  for (const G &g : geos)
    for (int fmt : {0, 2, 3}) {
      // map sizes round every switch: the coarse path ends where a block's 8 columns (16 luma pixels for a decimated plane) meet a
      // third cell -- from pw / 16 to pw / 4 --, the dword path where they span 8 cells or more -- about pw, and pw / 2 for chroma
      std::vector<int> ws = {1, 2, 3, g.pw / 16, g.pw / 16 + 1, g.pw / 8 - 1, g.pw / 8, g.pw / 8 + 1, g.pw / 4, g.pw / 4 + 1, g.pw / 2 - 1, g.pw / 2,
                             g.pw / 2 + 1, g.pw - 1, g.pw, g.pw + 1, 2 * g.pw - 1, 2 * g.pw, 2 * g.pw + 1, 3 * g.pw + 5};
      std::vector<int> hs = {1, g.ph / 16 + 1, g.ph / 8, g.ph / 4 + 1, g.ph, 2 * g.ph + 1};
      for (int wm : ws)
        for (int hm : hs)
          for (int pad : {0, 1, 4})
            for (int off : {0, 1})
              for (int neg = 0; neg < 2; neg++) {
                if (wm < 1 || hm < 1) continue;
                lanes += run(g.fw, g.fh, fmt, g.px, g.py, g.pw, g.ph, wm, hm, pad, off, neg != 0, (cases & 1) != 0);
                cases++;
              }
    }
  // the longest maps a side allows
  lanes += run(64, 48, 0, 0, 0, 64, 48, 16384, 1, 0, 0, false, false);
  lanes += run(64, 48, 0, 0, 0, 64, 48, 1, 16384, 3, 1, true, true);
  // a 3840 x 2160 picture with a map at pixel resolution
  lanes += run(3840, 2176, 0, 0, 0, 3840, 2160, 3840, 2160, 0, 0, false, false);
  cases += 3;
  printf("ok: %ld cases, %ld lanes; no read outside a map's rows, no write outside the output\n", cases, lanes);
  return 0;
}
