// The level choice's programme (rdq_walk of theora_amd/csrc/thip_encode_rdq.h, with the indexing of its arrays) built for the host
// under AddressSanitizer and UBSan (tests/test_encoder_rdq_cpu.py compiles and runs this).  The arrays are laid out as one wave's in
// the kernel -- F and dd [16][65] int64, the choices [16][68] bytes, the levels in the four-lane kernels' rotated pieces -- and
// everything but the entries of the block at work is poisoned, so an index that leaves its block stops the program.  Every block
// with at most 12 non-zero levels is compared with a brute force over all 2^n choices in lexicographic order; the heaviest block
// (all 63 positions +-1) and dense blocks are checked for J_after <= J_before, J_after = the J of the levels written, zeros that
// stay zero and a DC left alone.
#include <sanitizer/asan_interface.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#define THIP_RDQ_WALK_ONLY
#include "thip_encode_rdq.h"   // (-I theora_amd/csrc)
using namespace thip;

// the kernels' layout of a wave's levels (thip_fdct.h: lds_block_piece, lds_block_at), restated
static int piece(int bb, int pc) { return bb * 8 + ((pc + bb) & 7); }
static int at(int b, int z) { return piece(b, z >> 3) * 8 + (z & 7); }

static uint8_t g_bits[4][32];
static int grp(int zs) { return zs <= 5 ? 0 : zs <= 14 ? 1 : zs <= 27 ? 2 : 3; }
static int value_token(int v) {
  const int a = abs(v);
  if (a == 1) return 9 + (v < 0);
  if (a == 2) return 11 + (v < 0);
  if (a <= 6) return 10 + a;
  return a <= 8 ? 17 : a <= 12 ? 18 : a <= 20 ? 19 : a <= 36 ? 20 : a <= 68 ? 21 : 22;
}
// the header's token rule: the bits of v at z when the previous token ended before nxt
static int vbits(int v, int z, int nxt) {
  const int gap = z - nxt, a = abs(v);
  if (a == 1 && gap >= 1 && gap <= 17) return g_bits[grp(nxt)][gap <= 5 ? 22 + gap : gap <= 9 ? 28 : 29];
  if ((a == 2 || a == 3) && gap >= 1 && gap <= 3) return g_bits[grp(nxt)][gap == 1 ? 30 : 31];
  return (gap > 0 ? g_bits[grp(nxt)][gap <= 8 ? 7 : 8] : 0) + g_bits[grp(z)][value_token(v)];
}
static int ebits(int nxt) { return g_bits[grp(nxt)][0]; }
static int64_t rate(const int *l) {
  int64_t r = 0;
  int nxt = 1;
  for (int z = 1; z < 64; z++)
    if (l[z]) { r += vbits(l[z], z, nxt); nxt = z + 1; }
  return r + (nxt < 64 ? ebits(nxt) : 0);
}
static int64_t dist(const int *c, const int *l, const int *s) {
  int64_t d = 0;
  for (int z = 1; z < 64; z++) { const int64_t e = (int64_t)c[z] - (int64_t)l[z] * s[z]; d += e * e; }
  return d;
}
static int alt(int v) { return v - (v > 0 ? 1 : -1); }

struct Wave {
  std::vector<int64_t> F, dd;
  std::vector<uint8_t> ch;
  std::vector<int16_t> lv;
  Wave() : F(16 * kRdqStride), dd(16 * kRdqStride), ch(16 * kRdqChoiceStride), lv(16 * 64) {}
  void only(int b) {   // everything poisoned but block b's entries
    ASAN_POISON_MEMORY_REGION(F.data(), F.size() * 8);
    ASAN_POISON_MEMORY_REGION(dd.data(), dd.size() * 8);
    ASAN_POISON_MEMORY_REGION(ch.data(), ch.size());
    ASAN_POISON_MEMORY_REGION(lv.data(), lv.size() * 2);
    ASAN_UNPOISON_MEMORY_REGION(&F[rdq_at(b, 0)], 64 * 8);
    ASAN_UNPOISON_MEMORY_REGION(&dd[rdq_at(b, 0)], 64 * 8);
    ASAN_UNPOISON_MEMORY_REGION(&ch[rdq_choice_at(b, 0)], 64);
    for (int pc = 0; pc < 8; pc++) ASAN_UNPOISON_MEMORY_REGION(&lv[piece(b, pc) * 8], 16);
  }
  void all() {
    ASAN_UNPOISON_MEMORY_REGION(F.data(), F.size() * 8);
    ASAN_UNPOISON_MEMORY_REGION(dd.data(), dd.size() * 8);
    ASAN_UNPOISON_MEMORY_REGION(ch.data(), ch.size());
    ASAN_UNPOISON_MEMORY_REGION(lv.data(), lv.size() * 2);
  }
};

// one block through rdq_walk as the kernel calls it; returns J_after - the squared error of the levels as they came
static int64_t run(Wave &w, int b, const int *c, int *l, const int *s, int64_t lam, RdqCount &cnt) {
  w.only(b);
  uint64_t nzm = 0;
  for (int z = 1; z < 64; z++) {
    w.lv[at(b, z)] = (int16_t)l[z];
    if (!l[z]) continue;
    nzm |= 1ull << z;
    const int64_t e0 = (int64_t)c[z] - (int64_t)l[z] * s[z], e1 = (int64_t)c[z] - (int64_t)alt(l[z]) * s[z];
    w.dd[rdq_at(b, z)] = e1 * e1 - e0 * e0;
  }
  w.lv[at(b, 0)] = (int16_t)l[0];
  const int64_t f0 = rdq_walk(nzm, lam, w.F.data(), w.dd.data(), w.ch.data(), b, [&](int z) { return (int)w.lv[at(b, z)]; },
                              [&](int z, int v) { w.lv[at(b, z)] = (int16_t)v; }, vbits, ebits, cnt);
  for (int z = 0; z < 64; z++) l[z] = w.lv[at(b, z)];
  w.all();
  return f0;
}

static long g_fail = 0;
#define CHECK(x) do { if (!(x)) { g_fail++; fprintf(stderr, "line %d: %s (case %ld)\n", __LINE__, #x, cases); } } while (0)

int main() {
  Wave w;
  long cases = 0, changed = 0;
  srand(7);
  auto rnd = [](int lo, int hi) { return lo + rand() % (hi - lo + 1); };
  for (int table = 0; table < 3; table++) {
    for (int g = 0; g < 4; g++)
      for (int t = 0; t < 32; t++) g_bits[g][t] = table == 0 ? 6 : (uint8_t)rnd(1, 24);   // table 0: flat, ties everywhere
    for (int it = 0; it < 1500; it++, cases++) {
      int c[64] = {0}, l[64] = {0}, s[64], was[64];
      for (int z = 0; z < 64; z++) s[z] = rnd(4, 200);
      const int kind = it % 6, n = kind == 5 ? 63 : kind == 4 ? rnd(13, 40) : rnd(0, 12);
      for (int q = 0; q < n; q++) {
        const int z = kind == 5 ? 1 + q : rnd(1, 63);
        static const int mags[] = {1, 1, 1, 1, 2, 2, 3, 4, 6, 7, 8, 9, 12, 13, 20, 21, 36, 37, 68, 69, 600};
        l[z] = (kind == 5 ? 1 : mags[rnd(0, it % 3 ? 6 : 20)]) * (rand() & 1 ? 1 : -1);
      }
      if (it % 7 == 0) { memset(l, 0, sizeof(l)); l[rnd(1, 3)] = 2; l[rnd(0, 1) ? 62 : 63] = rand() & 1 ? 1 : -1; }   // a last level at 62, 63
      if (it % 11 == 0) { const int z0 = rnd(1, 40); for (int z = z0; z < z0 + 18 && z < 63; z++) l[z] = 0; }           // runs of 17 / 18
      l[0] = rnd(-300, 300);
      for (int z = 1; z < 64; z++) c[z] = l[z] * s[z] + rnd(-s[z], s[z]) * (it % 5 ? 1 : 3) / 2;
      const int64_t lams[] = {1, 7, 60, 500, 4000, (int64_t)1 << 40};
      const int64_t lam = lams[rnd(0, 5)];
      memcpy(was, l, sizeof(l));
      const int b = rnd(0, 15);
      RdqCount cnt;
      const int64_t jb = dist(c, was, s) + lam * rate(was), ja = dist(c, was, s) + run(w, b, c, l, s, lam, cnt);
      int nzero = 0, nlow = 0, nn = 0, nzpos[64];
      for (int z = 1; z < 64; z++) {
        if (was[z]) nzpos[nn++] = z;
        CHECK(was[z] != 0 || l[z] == 0);
        CHECK(l[z] == was[z] || l[z] == alt(was[z]));
        nzero += was[z] && !l[z];
        nlow += l[z] && l[z] != was[z];
      }
      CHECK(l[0] == was[0] && ja <= jb && ja == dist(c, l, s) + lam * rate(l) && cnt.zeroed == nzero && cnt.lowered == nlow);
      changed += nzero + nlow > 0;
      if (nn > 12) continue;
      int64_t best = 0;
      int bl[64];
      for (uint32_t m = 0; m < (1u << nn); m++) {   // m's bits from the top: a in lexicographic order
        int cand[64];
        memcpy(cand, was, sizeof(was));
        for (int q = 0; q < nn; q++)
          if (m >> (nn - 1 - q) & 1) cand[nzpos[q]] = alt(was[nzpos[q]]);
        const int64_t j = dist(c, cand, s) + lam * rate(cand);
        if (m == 0 || j < best) { best = j; memcpy(bl, cand, sizeof(cand)); }
      }
      CHECK(best == ja && !memcmp(bl, l, sizeof(bl)));
    }
  }
  printf("%ld cases, %ld changed, %ld failures\n", cases, changed, g_fail);
  return g_fail || changed < cases / 4 ? 1 : 0;
}
