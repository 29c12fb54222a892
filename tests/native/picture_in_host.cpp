// k_picture_in's body (theora_amd/csrc/thip_picture_in.h) built for the host, lane by lane, under AddressSanitizer and UBSan
// (tests/test_picture_in_cpu.py compiles and runs this): every byte outside the source rows and the destination rectangles is
// poisoned, so a load that leaves its row, a store that leaves its rectangle or a 16-byte access that is not aligned stops the
// program; the planes are compared with a plain restatement of include/theora_hip.h's definition.
#include <sanitizer/asan_interface.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
struct uint4 { uint32_t x, y, z, w; };
struct uint2 { uint32_t x, y; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return {a, b}; }
using std::max;
using std::min;
#define THIP_MAX_BATCH 8
#define THIP_PIC_YCBCR 0
#define THIP_PIC_RGB24 1
#define THIP_PIC_RGBA32 2
#define THIP_PIC_RGB_PLANAR 3
#define __builtin_amdgcn_alignbyte(a, b, c) 0u   // (k_picture_out's loads: not run here)
static struct { unsigned x, y; } blockIdx, threadIdx;
#include "thip_picture.h"   // (-I theora_amd/csrc): pic_byte, pic_store
#include "thip_picture_in.h"

struct Buf {   // rows x rb bytes at pitch, first byte `off` into a 64-byte guard; everything else poisoned
  std::vector<uint8_t> mem; uint8_t *base; int rows, rb; int64_t pitch;
  Buf(int rows_, int rb_, int pad, int off) : rows(rows_), rb(rb_), pitch(rb_ + pad) {
    mem.resize(128 + 16 + off + (size_t)rows * pitch, 0xA5);
    uintptr_t a = ((uintptr_t)mem.data() + 64 + 15) & ~(uintptr_t)15;
    base = (uint8_t *)a + off;
    ASAN_POISON_MEMORY_REGION(mem.data(), mem.size());
    for (int y = 0; y < rows; y++) ASAN_UNPOISON_MEMORY_REGION(base + y * pitch, rb);
  }
  ~Buf() { ASAN_UNPOISON_MEMORY_REGION(mem.data(), mem.size()); }
};

int main() {
  long cases = 0;
  for (int fmt = 1; fmt <= 3; fmt++) for (int pf : {0, 2, 3}) for (int w : {1, 2, 15, 16, 17, 32, 33, 48}) for (int h : {1, 2, 3, 9})
  for (int px = 0; px < 3; px++) for (int py = 0; py < 3; py++) for (int pad : {0, 5}) for (int off : {0, 1}) {
    const int hd = !(pf & 1), vd = !(pf & 2), bpp = fmt == 1 ? 3 : fmt == 2 ? 4 : 1, ns = fmt == 3 ? 3 : 1;
    const int cx0 = px >> hd, cy0 = py >> vd, cw = ((px + w + hd) >> hd) - cx0, ch = ((py + h + vd) >> vd) - cy0;
    std::vector<Buf *> S, D;
    for (int p = 0; p < ns; p++) S.push_back(new Buf(h, w * bpp, pad, off));
    D.push_back(new Buf(h, w, pad, off)); D.push_back(new Buf(ch, cw, pad, off)); D.push_back(new Buf(ch, cw, pad, off));
    for (auto b : S) for (int y = 0; y < h; y++) for (int x = 0; x < b->rb; x++) b->base[y * b->pitch + x] = (uint8_t)rand();
    PicInBatchK B; memset(&B, 0, sizeof(B));
    PicInReqK &K = B.r[0];
    K.format = fmt; K.hdec = hd; K.vdec = vd; K.ox = px & hd; K.oy = py & vd; K.w = w; K.h = h; K.cw = cw; K.ch = ch;
    K.cpr = hd ? (cw + 7) >> 3 : (cw + 15) >> 4; K.units = K.cpr * ch;
    for (int p = 0; p < 3; p++) { if (p < ns) { K.src[p] = S[p]->base; K.spitch[p] = S[p]->pitch; } K.dst[p] = D[p]->base; K.dpitch[p] = D[p]->pitch; }
    for (unsigned b = 0; b * 256 < (unsigned)K.units + 256; b++) for (unsigned t = 0; t < 256; t++) { blockIdx.x = b; blockIdx.y = 0; threadIdx.x = t; k_picture_in(B); }
    auto pix = [&](int x, int y, int c) { x = min(max(x, 0), w - 1); y = min(max(y, 0), h - 1);
      return fmt == 3 ? (int)S[c]->base[y * S[c]->pitch + x] : (int)S[0]->base[y * S[0]->pitch + x * bpp + c]; };
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
      int want = 16 + ((16829 * pix(x, y, 0) + 33039 * pix(x, y, 1) + 6416 * pix(x, y, 2) + 32768) >> 16);
      if (D[0]->base[y * D[0]->pitch + x] != want) { printf("luma mismatch fmt %d pf %d w %d h %d px %d py %d at %d,%d\n", fmt, pf, w, h, px, py, x, y); return 1; } }
    const int s = hd + vd;
    for (int j = 0; j < ch; j++) for (int i = 0; i < cw; i++) {
      int sr = 0, sg = 0, sb = 0;
      for (int dy = 0; dy <= vd; dy++) for (int dx = 0; dx <= hd; dx++) { int X = ((cx0 + i) << hd) + dx - px, Y = ((cy0 + j) << vd) + dy - py; sr += pix(X, Y, 0); sg += pix(X, Y, 1); sb += pix(X, Y, 2); }
      int cb = 128 + ((-9714 * sr - 19070 * sg + 28784 * sb + (1 << (15 + s))) >> (16 + s)), cr = 128 + ((28784 * sr - 24103 * sg - 4681 * sb + (1 << (15 + s))) >> (16 + s));
      if (D[1]->base[j * D[1]->pitch + i] != cb || D[2]->base[j * D[2]->pitch + i] != cr) { printf("chroma mismatch fmt %d pf %d w %d h %d px %d py %d at %d,%d\n", fmt, pf, w, h, px, py, i, j); return 1; } }
    for (auto b : S) delete b; for (auto b : D) delete b;
    cases++;
  }
  printf("ok: %ld cases, no read outside a source row, no write outside a destination rectangle\n", cases);
  return 0;
}
