// thip_bitstream.h -- what a Theora encoder and a decoder must agree on, stated once for the decoder's front end (thip_frontend.cpp)
// and the encoder's host side (thip_encode.hip): the tables of the specification (doc/spec/spec.tex, section and table numbers
// below), a frame's geometry, the quantisation matrix, the run-length codes and the motion-vector code.  Plain C++, no HIP: the
// front end and its native test driver build for the CPU.  The device forms of the Hilbert curve (thip_kernels.h, thip_costmaps.h)
// are not here.
#pragma once
#include <stdint.h>

#include <vector>

namespace thip {

inline int ilog(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }   // bits needed to store v (spec 1.4)

// zig-zag index -> natural position (spec Figure "zig-zag order")
const uint8_t kZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// extra bits that follow each DCT token (Tables 7.33 / 7.38)
const uint8_t kTokExtraBits[32] = {0, 0, 0, 2, 3, 4, 12, 3, 6, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 4, 5, 6, 10, 1, 1, 1, 1, 1, 3, 4, 2, 3};
// Table 7.19: mode alphabets of schemes 1..6 (code index -> mode), and the modes' numbers (Table 7.18)
const uint8_t kModeAlphabets[6][8] = {{3, 4, 2, 0, 1, 5, 6, 7}, {3, 4, 0, 2, 1, 5, 6, 7}, {3, 2, 4, 0, 1, 5, 6, 7},
                                      {3, 2, 0, 4, 1, 5, 6, 7}, {0, 3, 4, 2, 1, 5, 6, 7}, {0, 5, 3, 4, 2, 1, 6, 7}};
enum { MODE_INTER_NOMV = 0, MODE_INTRA = 1, MODE_INTER_MV = 2, MODE_INTER_MV_LAST = 3, MODE_INTER_MV_LAST2 = 4,
       MODE_GOLDEN_NOMV = 5, MODE_GOLDEN_MV = 6, MODE_INTER_MV_FOUR = 7 };
// (row, col) of the k-th block of a super block in coded (Hilbert) order (spec Figure 2.4)
const uint8_t kHilbert[16][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 0}, {2, 0}, {3, 0}, {3, 1}, {2, 1},
                                 {2, 2}, {3, 2}, {3, 3}, {2, 3}, {1, 3}, {1, 2}, {0, 2}, {0, 3}};
// macro blocks of a super block in coded order: (row, col) in units of macro blocks (spec Figure 2.5)
const uint8_t kMbOrder[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};

// ---- geometry (spec 2.3 - 2.4): planes, coded order, super blocks, macro blocks; rows count from the bottom ----------------------
struct MacroBlock {
  int32_t luma[4];     // fragment indices in raster order (A,B,C,D)
  int32_t chroma[2][4];   // slot = row * 2 + col of the macro block, -1 where the plane has no block
  int nchroma;         // chroma blocks per plane in this macro block
  int32_t raster;      // its index in raster order
};
struct FrameGeometry {
  int hdec, vdec;
  int nh[3], nv[3], fro[3], nfrags_pl[3];   // fragments across and down, first fragment and fragment count of each plane
  int nfrags;
  std::vector<int32_t> coded_order;      // all fragments, coded order, planes concatenated
  std::vector<int32_t> sb_start;         // per super block (all planes): first index in coded_order, +1 sentinel
  int nsbs;
  std::vector<MacroBlock> mbs;           // macro blocks in coded order (frame sizes are multiples of 16: whole ones only)
};
inline void build_geometry(FrameGeometry &g, int frame_width, int frame_height, int pixel_fmt) {
  g.hdec = !(pixel_fmt & 1);
  g.vdec = !(pixel_fmt & 2);
  const int yh = frame_width >> 3, yv = frame_height >> 3;
  g.nfrags = 0;
  for (int p = 0; p < 3; p++) {
    g.nh[p] = p ? (yh + g.hdec) >> g.hdec : yh;
    g.nv[p] = p ? (yv + g.vdec) >> g.vdec : yv;
    g.fro[p] = g.nfrags;
    g.nfrags_pl[p] = g.nh[p] * g.nv[p];
    g.nfrags += g.nfrags_pl[p];
  }
  g.coded_order.clear();
  g.sb_start.clear();
  for (int p = 0; p < 3; p++)
    for (int sby = 0; sby < g.nv[p]; sby += 4)
      for (int sbx = 0; sbx < g.nh[p]; sbx += 4) {
        g.sb_start.push_back((int32_t)g.coded_order.size());
        for (int k = 0; k < 16; k++) {
          const int by = sby + kHilbert[k][0], bx = sbx + kHilbert[k][1];
          if (by < g.nv[p] && bx < g.nh[p]) g.coded_order.push_back(g.fro[p] + by * g.nh[p] + bx);
        }
      }
  g.nsbs = (int)g.sb_start.size();
  g.sb_start.push_back((int32_t)g.coded_order.size());
  // macro blocks: luma super blocks in raster order, four macro blocks each in coded order
  g.mbs.clear();
  for (int sby = 0; sby < yv; sby += 4)
    for (int sbx = 0; sbx < yh; sbx += 4)
      for (int k = 0; k < 4; k++) {
        const int my = sby + 2 * kMbOrder[k][0], mx = sbx + 2 * kMbOrder[k][1];
        if (my >= yv || mx >= yh) continue;
        MacroBlock mb;
        mb.raster = (my >> 1) * (yh >> 1) + (mx >> 1);
        for (int i = 0; i < 2; i++)
          for (int j = 0; j < 2; j++) mb.luma[i * 2 + j] = (my + i) * yh + mx + j;
        const int cx = mx >> g.hdec, cy = my >> g.vdec;
        const int ncx = g.hdec ? 1 : 2, ncy = g.vdec ? 1 : 2;
        mb.nchroma = ncx * ncy;
        for (int c = 0; c < 2; c++) {
          // raster order inside the macro block; slot = i*2+j so that 4:4:4 lines up with
          // luma A,B,C,D and 4:2:2 uses slots 0 (bottom) and 2 (top)
          for (int i = 0; i < 4; i++) mb.chroma[c][i] = -1;
          for (int i = 0; i < ncy; i++)
            for (int j = 0; j < ncx; j++) mb.chroma[c][i * 2 + j] = g.fro[1 + c] + (cy + i) * g.nh[1] + cx + j;
        }
        g.mbs.push_back(mb);
      }
}

// ---- quantisation (spec 6.4.1 - 6.4.3): the setup header's parameters and the matrix they give ------------------------------------
struct QuantParams {
  uint8_t lflims[64];
  uint16_t acscale[64], dcscale[64];
  int nbms;
  std::vector<uint8_t> bms;   // nbms*64, natural order
  int nqrs[2][3];             // per (qti, pli): the quant ranges, their sizes, the base matrix at each of their nqrs + 1 ends
  int qrsizes[2][3][64];
  int qrbmis[2][3][65];
};
// spec 6.4.3 "Computing a Quantization Matrix"; output in ZIG-ZAG order
inline void compute_qmat(const QuantParams &q, int qti, int pli, int qi, uint16_t out_zz[64]) {
  int qri = 0, qistart = 0;
  while (qri < q.nqrs[qti][pli] - 1 && qi > qistart + q.qrsizes[qti][pli][qri]) {
    qistart += q.qrsizes[qti][pli][qri];
    qri++;
  }
  const int size = q.qrsizes[qti][pli][qri];
  const int qiend = qistart + size;
  const uint8_t *bmi = &q.bms[(size_t)q.qrbmis[qti][pli][qri] * 64];
  const uint8_t *bmj = &q.bms[(size_t)q.qrbmis[qti][pli][qri + 1] * 64];
  for (int zzi = 0; zzi < 64; zzi++) {
    const int ci = kZigZag[zzi];
    const int bm = (2 * (qiend - qi) * bmi[ci] + 2 * (qi - qistart) * bmj[ci] + size) / (2 * size);
    const int qmin = ci == 0 ? (qti == 0 ? 16 : 32) : (qti == 0 ? 8 : 16);
    const int qscale = ci == 0 ? q.dcscale[qi] : q.acscale[qi];
    int v = (qscale * bm / 100) * 4;
    if (v > 4096) v = 4096;
    if (v < qmin) v = qmin;
    out_zz[zzi] = (uint16_t)v;
  }
}

// ---- run-length codes of bit strings (spec 7.2): Table 7.7 (long runs) and Table 7.11 (short runs) ---------------------------------
// A run of class k is `start` plus `bits` further bits.  The prefix of class k is k ones and a zero, of the last class all ones.
struct RunCode {
  int last;   // the last class
  struct { uint16_t start; uint8_t bits; } cls[7];
  constexpr int longest() const { return cls[last].start + (1 << cls[last].bits) - 1; }
};
constexpr RunCode kLongRuns = {6, {{1, 0}, {2, 1}, {4, 1}, {6, 2}, {10, 3}, {18, 4}, {34, 12}}};
constexpr RunCode kShortRuns = {5, {{1, 1}, {3, 1}, {5, 1}, {7, 2}, {11, 2}, {15, 4}}};

// ---- motion-vector components in scheme 0 (spec 7.5.1, Table 7.23) ----------------------------------------------------------------
// A 3-bit prefix names the class: `bits` bits of magnitude above `base`, then a sign bit where there is one.  Eight bits at most,
// so the reader looks (value, length) up by the next eight bits; the writer looks (code, length) up by the component, -31..31.
struct MvVlc {
  int8_t value[256];
  uint8_t len[256];
  uint8_t code[63], nbits[63];   // of component v at v + 31
  MvVlc() {
    static const struct { int8_t base; uint8_t bits, sign; } kClass[8] = {{0, 0, 0}, {1, 0, 0}, {-1, 0, 0}, {2, 0, 1},
                                                                         {3, 0, 1}, {4, 2, 1}, {8, 3, 1}, {16, 4, 1}};
    for (int p = 0; p < 8; p++)
      for (int m = 0; m < 1 << kClass[p].bits; m++)
        for (int s = 0; s <= kClass[p].sign; s++) {
          const int v = s ? -(kClass[p].base + m) : kClass[p].base + m, n = 3 + kClass[p].bits + kClass[p].sign;
          const int cw = ((p << kClass[p].bits | m) << kClass[p].sign) | s;
          code[v + 31] = (uint8_t)cw;
          nbits[v + 31] = (uint8_t)n;
          for (int w = cw << (8 - n); w < (cw + 1) << (8 - n); w++) {
            value[w] = (int8_t)v;
            len[w] = (uint8_t)n;
          }
        }
  }
};
const MvVlc kMvVlc;

}  // namespace thip
