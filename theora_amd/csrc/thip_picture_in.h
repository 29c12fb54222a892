// k_picture_in: an R'G'B' picture in caller device memory turned into the picture-sized Y'CbCr planes the encoder takes
// (include/theora_hip.h, thip_picture_in): the integer matrix and the box mean over the 1 << (hdec + vdec) pixels of a chroma
// sample, the picture's edge repeated.  Included from thip_decode.hip behind thip_picture.h, whose stores it uses.
//
// One lane owns a run of chroma columns of one chroma row and the luma they cover: with hdec, 8 chroma columns and the 16 luma
// columns [16k, 16k + 16) of 1 + vdec rows; without, 16 columns of one row.  The luma chunk is aligned to the picture, not to the
// pairing: with an odd pic_x chroma column i covers picture columns 2i - 1 and 2i, so the lane reads one more pixel, 16k - 1, for
// its first pair and leaves pixel 16k + 15 to its neighbour's.  A chunk that lies whole inside its row and starts on 16 bytes
// is read with 16-byte loads; any other pixel by pixel, the column clamped to the picture.  Every read stays inside the source row
// it belongs to, rows are clamped to the picture before they are addressed.  No LDS, no scratch: every register array below is
// indexed with constants only.

struct PicInReqK {
  const uint8_t *src[3];
  uint8_t *dst[3];
  int64_t spitch[3], dpitch[3];
  int format, hdec, vdec;
  int ox, oy;          // pic_x & hdec, pic_y & vdec: the pairing's offset
  int w, h, cw, ch;    // the picture; the chroma region (plane 0 of the destination is w x h)
  int cpr, units;      // lanes per chroma row, lanes of the request
};
struct PicInBatchK {
  PicInReqK r[THIP_MAX_BATCH];
};

// The library's integer R'G'B' -> Y'CbCr (include/theora_hip.h states it); sums over 1 << s pixels for the chroma
__device__ __forceinline__ uint32_t pic_in_luma(int R, int G, int B) { return (uint32_t)(16 + ((16829 * R + 33039 * G + 6416 * B + 32768) >> 16)); }
__device__ __forceinline__ uint32_t pic_in_cb(int R, int G, int B, int s) {
  return (uint32_t)(128 + ((-9714 * R - 19070 * G + 28784 * B + (1 << (15 + s))) >> (16 + s)));
}
__device__ __forceinline__ uint32_t pic_in_cr(int R, int G, int B, int s) {
  return (uint32_t)(128 + ((28784 * R - 24103 * G - 4681 * B + (1 << (15 + s))) >> (16 + s)));
}

// one pixel of a source row, the column inside the picture
template <int FMT>
__device__ __forceinline__ void pic_in_pixel(const uint8_t *r0, const uint8_t *r1, const uint8_t *r2, int x, int &R, int &G, int &B) {
  if (FMT == THIP_PIC_RGB_PLANAR) {
    R = r0[x];
    G = r1[x];
    B = r2[x];
  } else {
    const uint8_t *p = r0 + (FMT == THIP_PIC_RGBA32 ? 4 : 3) * x;
    R = p[0];
    G = p[1];
    B = p[2];
  }
}

// the 16 pixels at columns x0 .. x0 + 15 of one source row of w pixels, columns beyond the picture taking its last
template <int FMT>
__device__ __forceinline__ void pic_in_chunk(const uint8_t *r0, const uint8_t *r1, const uint8_t *r2, int x0, int w, int R[16], int G[16],
                                             int B[16]) {
  constexpr int BPP = FMT == THIP_PIC_RGBA32 ? 4 : FMT == THIP_PIC_RGB24 ? 3 : 1;
  const uint8_t *p0 = r0 + BPP * x0;
  bool fast = x0 + 16 <= w && (((uintptr_t)p0) & 15) == 0;
  if (FMT == THIP_PIC_RGB_PLANAR) fast = fast && ((((uintptr_t)(r1 + x0)) | ((uintptr_t)(r2 + x0))) & 15) == 0;
  if (fast) {
    if (FMT == THIP_PIC_RGB_PLANAR) {
      const uint4 a = *reinterpret_cast<const uint4 *>(p0), b = *reinterpret_cast<const uint4 *>(r1 + x0),
                  c = *reinterpret_cast<const uint4 *>(r2 + x0);
#pragma unroll
      for (int i = 0; i < 16; i++) {
        R[i] = (int)pic_byte(a, i);
        G[i] = (int)pic_byte(b, i);
        B[i] = (int)pic_byte(c, i);
      }
    } else {
      uint32_t d[4 * BPP];
#pragma unroll
      for (int q = 0; q < BPP; q++) {
        const uint4 v = reinterpret_cast<const uint4 *>(p0)[q];
        d[4 * q] = v.x;
        d[4 * q + 1] = v.y;
        d[4 * q + 2] = v.z;
        d[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int i = 0; i < 16; i++) {
        R[i] = (int)((d[(BPP * i) >> 2] >> (8 * ((BPP * i) & 3))) & 255u);
        G[i] = (int)((d[(BPP * i + 1) >> 2] >> (8 * ((BPP * i + 1) & 3))) & 255u);
        B[i] = (int)((d[(BPP * i + 2) >> 2] >> (8 * ((BPP * i + 2) & 3))) & 255u);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) pic_in_pixel<FMT>(r0, r1, r2, min(x0 + i, w - 1), R[i], G[i], B[i]);
  }
}

// n (<= 8) bytes of w[0..1] to d: one 8-byte store for a whole chunk in an aligned row, bytes otherwise
__device__ __forceinline__ void pic_in_store8(uint8_t *d, const uint32_t w[2], int n) {
  if (n == 8 && (((uintptr_t)d) & 7) == 0) *reinterpret_cast<uint2 *>(d) = make_uint2(w[0], w[1]);
  else pic_store_bytes(d, w, n, 8);
}

// chroma row j, lane k of its row
template <int FMT, int HDEC>
__device__ __forceinline__ void pic_in_lane(const PicInReqK &Q, int j, int k) {
  constexpr int NC = HDEC ? 8 : 16;   // chroma columns of the lane
  const int x0 = 16 * k, s = HDEC + Q.vdec;
  int SR[NC], SG[NC], SB[NC];
#pragma unroll
  for (int m = 0; m < NC; m++) SR[m] = SG[m] = SB[m] = 0;
#pragma unroll
  for (int r = 0; r < 2; r++) {
    if (r > Q.vdec) break;
    const int y = (j << Q.vdec) - Q.oy + r, yc = min(max(y, 0), Q.h - 1);
    const uint8_t *r0 = Q.src[0] + (int64_t)yc * Q.spitch[0];
    const uint8_t *r1 = FMT == THIP_PIC_RGB_PLANAR ? Q.src[1] + (int64_t)yc * Q.spitch[1] : r0;
    const uint8_t *r2 = FMT == THIP_PIC_RGB_PLANAR ? Q.src[2] + (int64_t)yc * Q.spitch[2] : r0;
    int R[16], G[16], B[16];
    pic_in_chunk<FMT>(r0, r1, r2, x0, Q.w, R, G, B);
    if (y == yc && x0 < Q.w) {   // a real picture row: its luma
      uint32_t wy[4];
#pragma unroll
      for (int q = 0; q < 4; q++)
        wy[q] = pic_in_luma(R[4 * q], G[4 * q], B[4 * q]) | pic_in_luma(R[4 * q + 1], G[4 * q + 1], B[4 * q + 1]) << 8 |
                pic_in_luma(R[4 * q + 2], G[4 * q + 2], B[4 * q + 2]) << 16 | pic_in_luma(R[4 * q + 3], G[4 * q + 3], B[4 * q + 3]) << 24;
      pic_store<4>(Q.dst[0] + (int64_t)y * Q.dpitch[0] + x0, wy, min(16, Q.w - x0));
    }
    if (!HDEC) {
#pragma unroll
      for (int m = 0; m < 16; m++) {
        SR[m] += R[m];
        SG[m] += G[m];
        SB[m] += B[m];
      }
    } else if (Q.ox) {   // chroma column 8k + m covers picture columns 16k + 2m - 1 and 16k + 2m
      int Re, Ge, Be;
      pic_in_pixel<FMT>(r0, r1, r2, min(max(x0 - 1, 0), Q.w - 1), Re, Ge, Be);
#pragma unroll
      for (int m = 0; m < NC; m++) {
        SR[m] += R[2 * m] + (m ? R[m ? 2 * m - 1 : 0] : Re);
        SG[m] += G[2 * m] + (m ? G[m ? 2 * m - 1 : 0] : Ge);
        SB[m] += B[2 * m] + (m ? B[m ? 2 * m - 1 : 0] : Be);
      }
    } else {
#pragma unroll
      for (int m = 0; m < NC; m++) {
        SR[m] += R[2 * m] + R[2 * m + 1];
        SG[m] += G[2 * m] + G[2 * m + 1];
        SB[m] += B[2 * m] + B[2 * m + 1];
      }
    }
  }
  uint32_t wb[NC / 4], wr[NC / 4];
#pragma unroll
  for (int q = 0; q < NC / 4; q++) {
    wb[q] = wr[q] = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      wb[q] |= pic_in_cb(SR[4 * q + t], SG[4 * q + t], SB[4 * q + t], s) << (8 * t);
      wr[q] |= pic_in_cr(SR[4 * q + t], SG[4 * q + t], SB[4 * q + t], s) << (8 * t);
    }
  }
  const int n = min(NC, Q.cw - NC * k);
  uint8_t *const db = Q.dst[1] + (int64_t)j * Q.dpitch[1] + NC * k, *const dr = Q.dst[2] + (int64_t)j * Q.dpitch[2] + NC * k;
  if constexpr (HDEC != 0) {
    pic_in_store8(db, wb, n);
    pic_in_store8(dr, wr, n);
  } else {
    pic_store<NC / 4>(db, wb, n);
    pic_store<NC / 4>(dr, wr, n);
  }
}

__global__ __launch_bounds__(256) void k_picture_in(const PicInBatchK B) {
  const PicInReqK &Q = B.r[blockIdx.y];
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);
  if (u >= Q.units) return;
  const int j = u / Q.cpr, k = u - j * Q.cpr;
#define PIC_IN(F_)                            \
  do {                                        \
    if (Q.hdec) pic_in_lane<F_, 1>(Q, j, k);  \
    else pic_in_lane<F_, 0>(Q, j, k);         \
  } while (0)
  if (Q.format == THIP_PIC_RGB24) PIC_IN(THIP_PIC_RGB24);
  else if (Q.format == THIP_PIC_RGBA32) PIC_IN(THIP_PIC_RGBA32);
  else PIC_IN(THIP_PIC_RGB_PLANAR);
#undef PIC_IN
}
