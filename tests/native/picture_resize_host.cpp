// k_picture_resize's body (theora_amd/csrc/thip_picture_resize.h) built for the host, lane by lane, under AddressSanitizer and
// UBSan (tests/test_picture_resize_cpu.py compiles and runs this): every byte outside the source rectangles' rows and the
// destination rectangles is poisoned, so a load that leaves its rectangle, a store that leaves its rectangle or a 16-byte access
// that is not aligned stops the program; the output is compared with a plain restatement of include/theora_hip.h's definition.
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
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
using std::max;
using std::min;
#define THIP_MAX_BATCH 8
#define THIP_PIC_YCBCR 0
#define THIP_PIC_RGB24 1
#define THIP_PIC_RGBA32 2
#define THIP_PIC_RGB_PLANAR 3
#define THIP_FILTER_BILINEAR 0
#define THIP_FILTER_AREA 1
#define THIP_ELEM_U8 0
#define THIP_ELEM_F16 1
#define THIP_ELEM_F32 2
#define __builtin_amdgcn_alignbyte(a, b, c) 0u   // (k_picture_out's loads: not run here)
static inline uint64_t __umul64hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }
// binary32 -> binary16 bits, round to nearest even (the device converts with one instruction; here by hand)
static uint32_t f16_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return sign | 0x7C00u | (a > 0x7F800000u ? 0x200u : 0u);
  if (a >= 0x477FF000u) return sign | 0x7C00u;                       // rounds to 2^16 or beyond: infinity
  if (a < 0x33000001u) return sign;                                  // at most half the smallest subnormal: zero
  int e = (int)(a >> 23) - 127;
  uint32_t m = (a & 0x7FFFFFu) | 0x800000u;                          // 1.m, 24 bits
  int shift = e >= -14 ? 13 : 13 + (-14 - e);                        // bits dropped
  uint32_t q = m >> shift, rest = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
  if (rest > halfway || (rest == halfway && (q & 1))) q++;
  // normal: q holds the hidden bit at 1 << 10 (a carry moves into the exponent by itself); subnormal: exponent field 0
  return sign | (e >= -14 ? (uint32_t)((e + 14) << 10) + q : q);
}
#define RSZ_F16_BITS(v) f16_bits(v)
static struct { unsigned x, y; } blockIdx, threadIdx;
#include "thip_picture.h"   // (-I theora_amd/csrc): pic_rgb, pic_store
#include "thip_picture_resize.h"

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
};

// ---- the definition, restated plainly -----------------------------------------------------------------------------------------
static int64_t floordiv(int64_t a, int64_t b) { int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
struct Plane { const Buf *b; int sw, sh; int at(int i, int j) const { return b->base[(int64_t)(sh - 1 - j) * b->pitch + i]; } };   // (rows bottom first)
static int want_bilinear(const Plane &s, int O, int Oh, int X, int Y) {
  int64_t px = std::min<int64_t>(std::max<int64_t>(floordiv(((2 * (int64_t)X + 1) * s.sw - O) * 128, O), 0), (s.sw - 1) * 256);
  int64_t py = std::min<int64_t>(std::max<int64_t>(floordiv(((2 * (int64_t)Y + 1) * s.sh - Oh) * 128, Oh), 0), (s.sh - 1) * 256);
  int i0 = (int)(px >> 8), fx = (int)(px & 255), i1 = min(i0 + 1, s.sw - 1), j0 = (int)(py >> 8), fy = (int)(py & 255), j1 = min(j0 + 1, s.sh - 1);
  return ((256 - fy) * ((256 - fx) * s.at(i0, j0) + fx * s.at(i1, j0)) + fy * ((256 - fx) * s.at(i0, j1) + fx * s.at(i1, j1)) + 32768) >> 16;
}
static int want_area(const Plane &s, int O, int Oh, int X, int Y) {
  uint64_t acc = 0, wsum = 0;
  for (int j = 0; j < s.sh; j++) for (int i = 0; i < s.sw; i++) {
    int64_t wx = std::min<int64_t>((int64_t)(X + 1) * s.sw, (int64_t)(i + 1) * O) - std::max<int64_t>((int64_t)X * s.sw, (int64_t)i * O);
    int64_t wy = std::min<int64_t>((int64_t)(Y + 1) * s.sh, (int64_t)(j + 1) * Oh) - std::max<int64_t>((int64_t)Y * s.sh, (int64_t)j * Oh);
    if (wx > 0 && wy > 0) { acc += (uint64_t)(wx * wy) * (uint64_t)s.at(i, j); wsum += (uint64_t)(wx * wy); }
  }
  const uint64_t D = (uint64_t)s.sw * s.sh;
  if (wsum != D) { printf("weights sum to %llu, not %llu\n", (unsigned long long)wsum, (unsigned long long)D); exit(1); }
  return (int)((acc + (D >> 1)) / D);
}
static int clamp255(int v) { return min(max(v, 0), 255); }
static float norm_f32(int c, float scale, float bias) { volatile float v = (float)c * scale; v = v + bias; return v; }

int main(int argc, char **argv) {   // an argument 0..5: that (format, element) pair alone, so that the test can run the six side by side
  const int only = argc > 1 ? atoi(argv[1]) : -1;
  long cases = 0, refused = 0;
  const float scale[3] = {1.0f / (255 * 0.229f), 1.0f / (255 * 0.224f), 1.0f / (255 * 0.225f)}, bias[3] = {-0.485f / 0.229f, -0.456f / 0.224f, -0.406f / 0.225f};
  for (int fmt = 0; fmt <= 3; fmt++) for (int elem = 0; elem <= (fmt == 3 ? 2 : 0); elem++) for (int pf : {0, 2, 3}) for (int filt = 0; filt <= 1; filt++)
  for (int w : {1, 2, 15, 16, 17, 33}) for (int h : {1, 2, 3, 9}) for (int o = 0; o < 3; o++)
  for (int ow : {1, 2, 15, 16, 17, 33}) for (int oh : {1, 3, 8}) for (int pad : {0, 5}) for (int off : {0, 1}) {
    if (only >= 0 && only != fmt + elem) continue;
    const int hd = !(pf & 1), vd = !(pf & 2), x = o, y = o;
    const int esz = elem == 2 ? 4 : elem == 1 ? 2 : fmt == 1 ? 3 : fmt == 2 ? 4 : 1, nd = fmt == 1 || fmt == 2 ? 1 : 3;
    PicRszBatchK B; memset(&B, 0, sizeof(B));
    PicRszReqK &K = B.r[0];
    K.format = fmt; K.filter = filt; K.elem = elem;
    std::vector<Buf *> S, D;
    Plane P[3]; int pow_[3], poh[3];
    bool cap = false; int units = 0;
    for (int p = 0; p < 3; p++) {
      const int h_ = p ? hd : 0, v_ = p ? vd : 0, rx = x >> h_, ry = y >> v_, sw = ((x + w + h_) >> h_) - rx, sh = ((y + h + v_) >> v_) - ry;
      pow_[p] = fmt == 0 ? (ow + h_) >> h_ : ow; poh[p] = fmt == 0 ? (oh + v_) >> v_ : oh;
      if (filt == 1 && (sw > 32 * pow_[p] || sh > 32 * poh[p])) cap = true;
      S.push_back(new Buf(sh, sw, pad, off));
      for (int j = 0; j < sh; j++) for (int i = 0; i < sw; i++) S[p]->base[j * S[p]->pitch + i] = (uint8_t)rand();
      P[p] = {S[p], sw, sh};
      K.src[p] = S[p]->base - rx; K.spitch[p] = (int)S[p]->pitch; K.ph[p] = ry + sh; K.rx[p] = rx; K.ry[p] = ry;   // (the plane ends with the rectangle's last row)
      rsz_prepare_axis(K.ax[p], sw, pow_[p]); rsz_prepare_axis(K.ay[p], sh, poh[p]); rsz_prepare_area(K, p, sw, sh);
      K.scale[p] = scale[p]; K.bias[p] = bias[p];
      const int cpr = (pow_[p] + 15) >> 4;
      if (p == 0) K.cpr = cpr; else K.ccpr = cpr;
      if (p == 0 || fmt == 0) units += cpr * poh[p];
      K.unit_end[p] = units;
    }
    if (cap) { refused++; for (auto b : S) delete b; continue; }   // (the library refuses these: THIP_EINVAL)
    for (int p = 0; p < nd; p++) {
      D.push_back(new Buf(poh[p], pow_[p] * esz, pad, elem == 2 && off ? 4 : off));
      K.dst[p] = D[p]->base; K.dpitch[p] = D[p]->pitch;
    }
    for (unsigned b = 0; b * 256 < (unsigned)units + 256; b++) for (unsigned t = 0; t < 256; t++) { blockIdx.x = b; blockIdx.y = 0; threadIdx.x = t; k_picture_resize(B); }
    auto fail = [&](const char *what, int p, int X, int Y) {
      printf("%s mismatch fmt %d elem %d pf %d filter %d rect %d,%d %dx%d out %dx%d pad %d off %d plane %d at %d,%d\n", what, fmt, elem, pf, filt, x, y, w, h, ow, oh, pad, off, p, X, Y);
      exit(1); };
    auto sample = [&](int p, int X, int Y) { return filt ? want_area(P[p], pow_[p], poh[p], X, Y) : want_bilinear(P[p], pow_[p], poh[p], X, Y); };
    if (fmt == 0) {
      for (int p = 0; p < 3; p++) for (int Y = 0; Y < poh[p]; Y++) for (int X = 0; X < pow_[p]; X++)
        if (D[p]->base[Y * D[p]->pitch + X] != sample(p, X, Y)) fail("plane", p, X, Y);
    } else {
      for (int Y = 0; Y < oh; Y++) for (int X = 0; X < ow; X++) {
        const int yy = 76309 * (sample(0, X, Y) - 16) + 32768, u = sample(1, X, Y) - 128, v = sample(2, X, Y) - 128;
        const int c[3] = {clamp255((yy + 104597 * v) >> 16), clamp255((yy - 25675 * u - 53279 * v) >> 16), clamp255((yy + 132201 * u) >> 16)};
        for (int k = 0; k < 3; k++) {
          if (fmt == 3) {
            const uint8_t *d = D[k]->base + Y * D[k]->pitch + X * esz;
            if (elem == 0) { if (d[0] != c[k]) fail("planar", k, X, Y); continue; }
            const float f = norm_f32(c[k], scale[k], bias[k]);
            uint32_t got = 0, wantbits;
            memcpy(&got, d, esz);
            if (elem == 2) memcpy(&wantbits, &f, 4); else wantbits = f16_bits(f);
            if (got != wantbits) fail("float", k, X, Y);
          } else if (D[0]->base[Y * D[0]->pitch + X * esz + k] != c[k]) fail("rgb", k, X, Y);
        }
        if (fmt == 2 && D[0]->base[Y * D[0]->pitch + X * 4 + 3] != 255) fail("alpha", 3, X, Y);
      }
    }
    for (auto b : S) delete b; for (auto b : D) delete b;
    cases++;
  }
  printf("ok: %ld cases, %ld beyond the area limit not run; no read outside a source rectangle, no write outside a destination rectangle\n", cases, refused);
  return 0;
}
