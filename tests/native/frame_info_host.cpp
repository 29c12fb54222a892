// k_frame_info's body (theora_amd/csrc/thip_frame_info.h) built for the host, lane by lane, under AddressSanitizer and UBSan
// (tests/test_frame_info_cpu.py compiles and runs this): every byte outside the source arrays and the destination rectangles is
// poisoned, so a load that leaves the frame's words, a store that leaves its rectangle or a 16-byte store that is not aligned stops
// the program; every output is compared with a plain loop over fragments and pixels.  k_frame_info_keep's body likewise.
//
//   frame_info_host 0 [pf]     every rectangle of a 40 x 24 frame, three pixel formats; the row alignment (0..15), the row padding,
//                              the element type and the source (tile-ordered frag_info / the record) change from one rectangle to
//                              the next, so that each is met many times over
//   frame_info_host 1 | 2 [pf] 40 x 24 | 136 x 72, three pixel formats: every column range (x, width) at every row alignment 0..15 in
//                              both element types, over two row ranges; and every row range (y, height) over four column ranges.
//                              (The kernel's row and column arithmetic do not meet: a lane's row picks the fragment row and the
//                              destination row, its chunk the columns.  Every rectangle of 136 x 72 -- 24 million -- is beyond a
//                              test.)
#include <sanitizer/asan_interface.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "theora_hip.h"   // (-I include): the command word's bits, THIP_ELEM_*, THIP_FI_REF_*
#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
using std::max;
using std::min;
#define __builtin_amdgcn_alignbyte(a, b, c) 0u   // (k_picture_out's loads: not run here)
// (row, col) of the h-th block of a super block along its Hilbert curve, written out from the specification's figure
static const int kCurve[16][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 0}, {2, 0}, {3, 0}, {3, 1}, {2, 1}, {2, 2}, {3, 2}, {3, 3}, {2, 3}, {1, 3}, {1, 2}, {0, 2}, {0, 3}};
static int hilb_row(int h) { return kCurve[h][0]; }
static int hilb_col(int h) { return kCurve[h][1]; }
static int hilb_inv(int r, int c) { for (int h = 0; h < 16; h++) if (kCurve[h][0] == r && kCurve[h][1] == c) return h; abort(); }
// binary32 -> binary16 bits for the values the field holds: multiples of 0.5 of magnitude at most 64, all exact
static uint32_t f16_exact(float f) {
  if (f == 0.0f) return 0;
  uint32_t x; memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u, e = ((x >> 23) & 255u) - 127u + 15u, m = x & 0x7FFFFFu;
  if (e < 1 || e > 30 || (m & 0x1FFFu)) abort();
  return sign | e << 10 | m >> 13;
}
#define FI_F16_BITS(v) f16_exact(v)
static struct { unsigned x, y; } blockIdx, threadIdx;
#include "thip_picture.h"   // (-I theora_amd/csrc): pic_store
#include "thip_frame_info.h"

struct Buf {   // rows x rb bytes at pitch, first byte `off` past a 16-byte boundary inside a guard; everything else poisoned
  std::vector<uint8_t> mem; uint8_t *base; int rows, rb; int64_t pitch;
  Buf(int rows_, int rb_, int pad, int off) : rows(rows_), rb(rb_), pitch(rb_ + pad) {
    mem.resize(128 + 16 + off + (size_t)rows * pitch, 0xA5);
    uintptr_t a = ((uintptr_t)mem.data() + 64 + 15) & ~(uintptr_t)15;
    base = (uint8_t *)a + off;
    ASAN_POISON_MEMORY_REGION(mem.data(), mem.size());
    for (int y = 0; y < rows; y++) ASAN_UNPOISON_MEMORY_REGION(base + y * pitch, rb);
  }
  ~Buf() { ASAN_UNPOISON_MEMORY_REGION(mem.data(), mem.size()); }
  uint8_t at(int row, int b) const { return base[row * pitch + b]; }
};

struct Frame {   // the geometry of thip_state_create, and a frame's words in raster order, in tile order and as the record
  int W, H, hd, vd, nh[3], nv[3], fro[3], tiles_x[3], tile_off[3], ntiles, nfrags;
  std::vector<uint32_t> w0;   // raster
  Buf *tiled, *rec;
  Frame(int W_, int H_, int pf) : W(W_), H(H_), hd(!(pf & 1)), vd(!(pf & 2)) {
    int f = 0, t = 0;
    for (int p = 0; p < 3; p++) {
      nh[p] = p ? ((W >> 3) + hd) >> hd : W >> 3; nv[p] = p ? ((H >> 3) + vd) >> vd : H >> 3;
      fro[p] = f; f += nh[p] * nv[p];
      tiles_x[p] = (nh[p] + 15) / 16; tile_off[p] = t; t += tiles_x[p] * ((nv[p] + 3) / 4);
    }
    nfrags = f; ntiles = t;
    w0.resize(nfrags);
    for (auto &w : w0) {   // every bit random: stale vectors on uncoded and intra fragments, dc_only and qii set or not; refi 0..2
      w = ((uint32_t)rand() << 16) ^ (uint32_t)rand();
      w &= ~(3u << THIP_INFO_REFI_SHIFT); w |= (uint32_t)(rand() % 3) << THIP_INFO_REFI_SHIFT;
      w &= ~(127u << THIP_INFO_LAST_ZZI_SHIFT); w |= (uint32_t)(rand() % 65) << THIP_INFO_LAST_ZZI_SHIFT;
      if (rand() % 3 == 0) w &= ~1u;
    }
    tiled = new Buf(1, ntiles * 64 * 8, 0, 0);
    memset(tiled->base, 0xEE, (size_t)ntiles * 64 * 8);   // (positions outside the planes and every word1: never looked at)
    rec = new Buf(1, nfrags * 4, 0, 0);
    uint32_t *ti = (uint32_t *)tiled->base;
    for (int p = 0; p < 3; p++) for (int by = 0; by < nv[p]; by++) for (int bx = 0; bx < nh[p]; bx++) {
      int h = -1;
      for (int k = 0; k < 16; k++) if (kCurve[k][0] == (by & 3) && kCurve[k][1] == (bx & 3)) h = k;
      const int pos = (tile_off[p] + (by >> 2) * tiles_x[p] + (bx >> 4)) * 64 + ((bx >> 2) & 3) * 16 + h;
      ti[2 * pos] = w0[fro[p] + by * nh[p] + bx];
    }
  }
  ~Frame() { delete tiled; delete rec; }
  uint32_t word(int p, int bx, int top_row) const { return w0[fro[p] + (nv[p] - 1 - top_row) * nh[p] + bx]; }   // top_row: from the top
};
static int kind_of(uint32_t w) { const int r = (w >> 1) & 3; return !(w & 1) ? 0 : r == THIP_FRAME_SELF ? 1 : r == THIP_FRAME_PREV ? 2 : 3; }
static int vx_of(uint32_t w) { return kind_of(w) >= 2 ? (int8_t)(w >> 16) : 0; }
static int vy_of(uint32_t w) { return kind_of(w) >= 2 ? (int8_t)(uint8_t)(-(int)(int8_t)(w >> 24)) : 0; }

static void run(const FiBatchK &B, int units) {
  for (unsigned b = 0; b * 256 < (unsigned)units + 256; b++) for (unsigned t = 0; t < 256; t++) { blockIdx.x = b; blockIdx.y = 0; threadIdx.x = t; k_frame_info(B); }
}
static long g_cases = 0;
// one request: the rectangle, the element type, refs, the row alignment and padding of every destination, the source
static void one(const Frame &F, int x, int y, int w, int h, int elem, int refs, int off, int pad, bool tiled, bool maps, bool dense) {
  FiBatchK B; memset(&B, 0, sizeof(B));
  FiReqK &K = B.r[0];
  K.tiled = tiled; K.info = (const uint32_t *)(tiled ? F.tiled->base : F.rec->base);
  K.elem = elem; K.refs = refs; K.x = x; K.y = y; K.w = w; K.h = h;
  const int esz = elem == THIP_ELEM_F32 ? 4 : 2;
  std::vector<Buf *> bufs;
  Buf *bk[3] = {}, *bm[3] = {}, *bn[3] = {}, *bf = nullptr, *bv = nullptr;
  int fc0[3], fr0[3], fw[3], fh[3], units = 0;
  for (int p = 0; p < 3; p++) {
    const int hd = p ? F.hd : 0, vd = p ? F.vd : 0;
    fc0[p] = (x >> hd) >> 3; fr0[p] = (y >> vd) >> 3;
    fw[p] = (((x + w - 1) >> hd) >> 3) - fc0[p] + 1; fh[p] = (((y + h - 1) >> vd) >> 3) - fr0[p] + 1;
    K.nh[p] = F.nh[p]; K.nv[p] = F.nv[p]; K.fro[p] = F.fro[p]; K.tiles_x[p] = F.tiles_x[p]; K.tile_off[p] = F.tile_off[p];
    K.fc0[p] = fc0[p]; K.fr0[p] = fr0[p]; K.fw[p] = fw[p];
    if (maps && (p != 1 || (g_cases & 1))) {   // (a plane whose maps are not wanted now and then)
      bufs.push_back(bk[p] = new Buf(fh[p], fw[p], pad, off)); bufs.push_back(bn[p] = new Buf(fh[p], fw[p], pad, (off + 3) & 15));
      bufs.push_back(bm[p] = new Buf(fh[p], 2 * fw[p], pad, (off + 7) & 15));
      K.kind[p] = bk[p]->base; K.kind_pitch[p] = bk[p]->pitch; K.ncoef[p] = bn[p]->base; K.ncoef_pitch[p] = bn[p]->pitch;
      K.mv[p] = bm[p]->base; K.mv_pitch[p] = bm[p]->pitch;
      if ((g_cases & 7) == 3) K.ncoef[p] = nullptr;   // (each pointer is optional by itself)
      units += fw[p] * fh[p];
    }
    K.unit_end[p] = units;
  }
  K.cpr_flow = (w * esz + 15) / 16 + 1; K.cpr_valid = (w + 15) / 16 + 1;
  if (dense) {
    bufs.push_back(bf = new Buf(2 * h, w * esz, pad, off)); bufs.push_back(bv = new Buf(h, w, pad, off));
    K.flow = bf->base; K.flow_pitch = bf->pitch; K.valid = bv->base; K.valid_pitch = bv->pitch;
    units += 2 * h * K.cpr_flow;
  }
  K.unit_end[3] = units;
  if (dense) units += h * K.cpr_valid;
  K.unit_end[4] = units;
  run(B, units);
  auto fail = [&](const char *what, int p, int X, int Y) {
    printf("%s mismatch: frame %dx%d hd %d vd %d rect %d,%d %dx%d elem %d refs %d off %d pad %d tiled %d plane %d at %d,%d\n", what, F.W, F.H, F.hd, F.vd, x, y, w, h,
           elem, refs, off, pad, (int)tiled, p, X, Y);
    exit(1); };
  for (int p = 0; p < 3; p++) {
    if (!bk[p]) continue;
    for (int r = 0; r < fh[p]; r++) for (int c = 0; c < fw[p]; c++) {
      const uint32_t wd = F.word(p, fc0[p] + c, fr0[p] + r);
      if (bk[p]->at(r, c) != kind_of(wd)) fail("kind", p, c, r);
      if (K.ncoef[p] ? bn[p]->at(r, c) != (kind_of(wd) ? (wd >> 8) & 127 : 0) : bn[p]->at(r, c) != 0xA5) fail("ncoef", p, c, r);
      if ((int8_t)bm[p]->at(r, 2 * c) != vx_of(wd) || (int8_t)bm[p]->at(r, 2 * c + 1) != vy_of(wd)) fail("mv", p, c, r);
    }
  }
  if (dense) for (int j = 0; j < h; j++) for (int i = 0; i < w; i++) {
    const uint32_t wd = F.word(0, (x + i) >> 3, (y + j) >> 3);
    const int k = kind_of(wd);
    if (bv->at(j, i) != k) fail("valid", 0, i, j);
    const bool on = (k == 2 && (refs & THIP_FI_REF_PREV)) || (k == 3 && (refs & THIP_FI_REF_GOLD));
    for (int c = 0; c < 2; c++) {
      const float want = on ? 0.5f * (float)(c ? vy_of(wd) : vx_of(wd)) : 0.0f;
      uint32_t got = 0, wb;
      memcpy(&got, bf->base + (c * h + j) * bf->pitch + i * esz, esz);
      if (esz == 4) memcpy(&wb, &want, 4); else wb = f16_exact(want);
      if (got != wb) fail("flow", c, i, j);
    }
  }
  for (auto b : bufs) delete b;
  g_cases++;
}

static void keep(Frame &F) {   // k_frame_info_keep: the record from the tile-ordered words
  FiKeepK K; memset(&K, 0, sizeof(K));
  K.info = (const uint32_t *)F.tiled->base; K.rec = (uint32_t *)F.rec->base; K.npos = F.ntiles * 64;
  for (int p = 0; p < 3; p++) { K.nh[p] = F.nh[p]; K.nv[p] = F.nv[p]; K.fro[p] = F.fro[p]; K.tiles_x[p] = F.tiles_x[p]; K.tile_off[p] = F.tile_off[p]; }
  memset(F.rec->base, 0x5A, (size_t)F.nfrags * 4);
  for (unsigned b = 0; b * 256 < (unsigned)K.npos + 256; b++) for (unsigned t = 0; t < 256; t++) { blockIdx.x = b; threadIdx.x = t; k_frame_info_keep(K); }
  for (int f = 0; f < F.nfrags; f++)
    if (((const uint32_t *)F.rec->base)[f] != ((F.w0[f] & 1) ? F.w0[f] & 0xFFFF7F07u : 0u)) { printf("record mismatch at fragment %d\n", f); exit(1); }
}

int main(int argc, char **argv) {
  const int mode = argc > 1 ? atoi(argv[1]) : 0, only = argc > 2 ? atoi(argv[2]) : -1;   // (a second argument: that pixel format alone)
  srand(1234 + mode);
  for (int pf : {0, 2, 3}) {
    if (only >= 0 && only != pf) continue;
    const int RW = mode == 2 ? 136 : 40, RH = mode == 2 ? 72 : 24;
    Frame F((RW + 15) & ~15, (RH + 15) & ~15, pf);   // (coded frames are multiples of 16: the rectangles lie in 48 x 32 and 144 x 80)
    keep(F);
    long n = 0;
    if (mode == 0) {
      for (int x = 0; x < RW; x++) for (int w = 1; x + w <= RW; w++) for (int y = 0; y < RH; y++) for (int h = 1; y + h <= RH; h++, n++)
        one(F, x, y, w, h, (n >> 4) & 1 ? THIP_ELEM_F32 : THIP_ELEM_F16, (int)((n >> 5) & 3), (int)(n & 15), (n >> 7) & 1 ? 5 : (16 - (w * ((n >> 4) & 1 ? 4 : 2)) % 16) % 16,
            (n >> 8) & 1, (n % 3) != 0, (n % 3) != 1);
    } else {
      const int ys[2][2] = {{0, 1}, {RH - 9, 2}};   // (the second one lies across two fragment rows)
      const int xs[4][2] = {{0, RW}, {3, 1}, {2, 37}, {RW - 9, 9}};
      for (int x = 0; x < RW; x++) for (int w = 1; x + w <= RW; w++) for (int off = 0; off < 16; off++) for (int e = 0; e < 2; e++, n++)
        one(F, x, ys[n & 1][0], w, ys[n & 1][1], e ? THIP_ELEM_F32 : THIP_ELEM_F16, (int)((n >> 1) & 3), off, (n >> 3) & 1 ? 5 : 0, (n >> 2) & 1, (n & 15) == 0, true);
      for (int y = 0; y < RH; y++) for (int h = 1; y + h <= RH; h++) for (int k = 0; k < 4; k++, n++)
        one(F, xs[k][0], y, xs[k][1], h, n & 1 ? THIP_ELEM_F32 : THIP_ELEM_F16, 3, (int)(n & 15), 5, (n >> 1) & 1, true, (n & 3) != 0);
    }
  }
  printf("ok: %ld requests; no read outside a frame's words, no write outside a destination rectangle\n", g_cases);
  return 0;
}
