// k_picture_compare's load-and-sum body (theora_amd/csrc/thip_picture_compare.h: cmp_load_rows, cmp_lane_cells, cmp_window_q20)
// built for the host, lane by lane, under AddressSanitizer and UBSan (tests/test_picture_compare_cpu.py compiles and runs this):
// every byte outside the two rectangles is poisoned, so a load that leaves its rectangle or a 16-byte / 4-byte load that is not
// aligned stops the program; the cell sums, the plane's squared differences and every window's w are compared with plain loops
// over include/theora_hip.h's definition.  The work-group part of the kernel (LDS, the reductions, the atomics) is not built here.
#include <sanitizer/asan_interface.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
struct alignas(16) uint4 { uint32_t x, y, z, w; };   // (16-byte alignment, as on the device: UBSan sees a 16-byte load that is not aligned)
using std::max;
using std::min;
#define THIP_MAX_BATCH 8
#define THIP_CMP_SSE 1
#define THIP_CMP_SSIM 2
struct thip_picture_metrics { int64_t sse[3], samples[3], ssim_q20[3], windows[3]; };
static inline uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) {   // v_dot4_u32_u8
  for (int k = 0; k < 4; k++) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
  return c;
}
#define CMP_DOT4(a, b, c) dot4((a), (b), (c))
#include "thip_picture_compare.h"   // (-I theora_amd/csrc)

struct Buf {   // rows x rb bytes at pitch, first byte `off` past a 16-byte boundary inside a guard; everything else poisoned
  std::vector<uint8_t> mem; uint8_t *base; int rows, rb; int64_t pitch;
  Buf(int rows_, int rb_, int pad, int off) : rows(rows_), rb(rb_), pitch(rb_ + pad) {
    mem.resize(128 + 16 + off + (size_t)rows * pitch, 0xA5);
    uintptr_t a = ((uintptr_t)mem.data() + 64 + 15) & ~(uintptr_t)15;
    base = (uint8_t *)a + off;
    for (int y = 0; y < rows; y++) for (int x = 0; x < rb; x++) base[y * pitch + x] = (uint8_t)rand();
    ASAN_POISON_MEMORY_REGION(mem.data(), mem.size());
    for (int y = 0; y < rows; y++) ASAN_UNPOISON_MEMORY_REGION(base + y * pitch, rb);
  }
  ~Buf() { ASAN_UNPOISON_MEMORY_REGION(mem.data(), mem.size()); }
};

static int64_t cdiv(int64_t n, int64_t d) { return n / d; }   // C's division: toward zero

int main(int argc, char **argv) {   // argv[1]: the pixel format (0, 2, 3), one process each
  const int pf = argc > 1 ? atoi(argv[1]) : 0;
  long cases = 0, windows = 0;
  uint32_t lcg = 12345;
  auto rnd16 = [&]() { lcg = lcg * 1664525u + 1013904223u; return (int)(lcg >> 24) & 15; };
  for (int w = 1; w <= 40; w++) for (int h = 1; h <= 40; h++) for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) {
    const int hd = !(pf & 1), vd = !(pf & 2);
    PicCmpReqK K; memset(&K, 0, sizeof(K));
    std::vector<Buf *> S, R;
    // Pitches (row + 0..15) and alignments (0..15 past a 16-byte boundary) of both sides.  By the case's number: 0 of 8 both sides
    // on 16 bytes with pitches that are multiples of 16 (16-byte loads on both sides wherever 16 columns fit), 1 the state's side
    // so and the other picture's drawn, 2 the reverse, 3 both on 4 bytes with pitches that are multiples of 4 (dword loads); the
    // other four drawn from a generator on both sides -- random coverage of the 16^4 combinations, not a walk through them.
    for (int p = 0; p < 3; p++) {
      const int phd = p ? hd : 0, pvd = p ? vd : 0;
      K.rx[p] = x >> phd; K.ry[p] = y >> pvd;
      K.sw[p] = ((x + w + phd) >> phd) - K.rx[p]; K.sh[p] = ((y + h + pvd) >> pvd) - K.ry[p];
      const int kind = (int)(cases & 7), a16 = (16 - (K.sw[p] & 15)) & 15, a4 = (4 - (K.sw[p] & 3)) & 3;
      int spad = rnd16(), soff = rnd16(), rpad = rnd16(), roff = rnd16();
      if (kind == 0 || kind == 1) { spad = a16; soff = 0; }
      if (kind == 0 || kind == 2) { rpad = a16; roff = 0; }
      if (kind == 3) { spad = a4 + 4 * (spad & 3); soff = 4 * (soff & 3); rpad = a4 + 4 * (rpad & 3); roff = 4 * (roff & 3); }
      S.push_back(new Buf(K.sh[p], K.sw[p], spad, soff));
      R.push_back(new Buf(K.sh[p], K.sw[p], rpad, roff));
      if ((cases + p) % 7 == 0) for (int j = 0; j < K.sh[p]; j++) memset(R[p]->base + j * R[p]->pitch, (cases & 1) ? 255 : 0, K.sw[p]);   // extremes
      if ((cases + p) % 7 == 0) for (int j = 0; j < K.sh[p]; j++) memset(S[p]->base + j * S[p]->pitch, (cases & 2) ? 0 : 255, K.sw[p]);
      // the state's plane is stored bottom row first: display row j of the rectangle is memory row ph - 1 - (ry + j)
      K.ph[p] = K.ry[p] + K.sh[p]; K.spitch[p] = (int)S[p]->pitch; K.src[p] = S[p]->base - K.rx[p];
      K.ref[p] = R[p]->base; K.rpitch[p] = R[p]->pitch;
    }
    for (int p = 0; p < 3; p++) {
      const int sw = K.sw[p], sh = K.sh[p], cw = (sw + 3) / 4 + 8, chh = (sh + 3) / 4 + 5;
      auto s = [&](int i, int j) { return (int64_t)S[p]->base[(sh - 1 - j) * S[p]->pitch + i]; };
      auto r = [&](int i, int j) { return (int64_t)R[p]->base[j * R[p]->pitch + i]; };
      std::vector<uint32_t> cells((size_t)5 * cw * chh, 0);
      int64_t sse = 0;
      for (int y0 = 0; y0 < sh + 8; y0 += 8) for (int x0 = 0; x0 < sw + 16; x0 += 16) {   // (one lane beyond each edge: it reads nothing)
        uint32_t C[5][8];
        cmp_lane_cells(K, p, x0, y0, C);
        for (int c = 0; c < 8; c++) {
          for (int q = 0; q < 5; q++) cells[((size_t)q * chh + y0 / 4 + c / 4) * cw + x0 / 4 + (c & 3)] = C[q][c];
          sse += (int64_t)(C[2][c] + C[3][c] - 2 * C[4][c]);
        }
      }
      int64_t want = 0;
      for (int j = 0; j < sh; j++) for (int i = 0; i < sw; i++) want += (s(i, j) - r(i, j)) * (s(i, j) - r(i, j));
      if (sse != want) { printf("sse mismatch pf %d w %d h %d x %d y %d plane %d\n", pf, w, h, x, y, p); return 1; }
      for (int cj = 0; cj < chh; cj++) for (int ci = 0; ci < cw; ci++) {
        int64_t v[5] = {0, 0, 0, 0, 0};
        for (int j = 4 * cj; j < min(4 * cj + 4, sh); j++) for (int i = 4 * ci; i < min(4 * ci + 4, sw); i++) {
          v[0] += s(i, j); v[1] += r(i, j); v[2] += s(i, j) * s(i, j); v[3] += r(i, j) * r(i, j); v[4] += s(i, j) * r(i, j); }
        for (int q = 0; q < 5; q++) if (cells[((size_t)q * chh + cj) * cw + ci] != v[q]) {
          printf("cell mismatch pf %d w %d h %d x %d y %d plane %d cell %d,%d sum %d\n", pf, w, h, x, y, p, ci, cj, q); return 1; }
      }
      for (int wy = 0; wy + 8 <= sh; wy += 4) for (int wx = 0; wx + 8 <= sw; wx += 4) {
        uint32_t t[5];
        for (int q = 0; q < 5; q++) { const uint32_t *c = &cells[((size_t)q * chh + wy / 4) * cw + wx / 4]; t[q] = c[0] + c[1] + c[cw] + c[cw + 1]; }
        int64_t sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int j = wy; j < wy + 8; j++) for (int i = wx; i < wx + 8; i++) { sx += s(i, j); sy += r(i, j); sxx += s(i, j) * s(i, j); syy += r(i, j) * r(i, j); sxy += s(i, j) * r(i, j); }
        const int64_t a = 2 * sx * sy + 26634, b = sx * sx + sy * sy + 26634, c = 2 * (64 * sxy - sx * sy) + 239708;
        const int64_t d = (64 * sxx - sx * sx) + (64 * syy - sy * sy) + 239708;
        const int64_t wq = cdiv(cdiv(a * 1048576, b) * cdiv(c * 1048576, d), 1048576);
        if (!(0 < a && a <= b && b < (1 << 29) && (c < 0 ? -c : c) <= d && d < (1 << 28))) { printf("bounds broken\n"); return 1; }
        if (cmp_window_q20(t[0], t[1], t[2], t[3], t[4]) != wq) { printf("window mismatch pf %d w %d h %d plane %d at %d,%d\n", pf, w, h, p, wx, wy); return 1; }
        windows++;
      }
    }
    for (auto b : S) delete b;
    for (auto b : R) delete b;
    cases++;
  }
  printf("ok: %ld cases, %ld windows, no read outside a rectangle\n", cases, windows);   // 40 * 40 * 4 * 4 cases
  return 0;
}
