// k_picture_out: a finished picture of a state, cropped, turned top row first and written to caller device memory as planar
// Y'CbCr or as R'G'B' (include/theora_hip.h, thip_picture_out).  Included from thip_decode.hip.
//
// One lane makes 16 consecutive pixels of one output row (for THIP_PIC_YCBCR: 16 bytes of one plane row) and writes them with
// 16-byte stores where the destination row allows it (a row whose start is 16-byte aligned; torch allocations are), byte by byte
// elsewhere.  Source rows are read with 16-byte loads where the crop keeps them aligned and as clamped aligned dwords put
// together with v_alignbyte_b32 otherwise (odd x); every read stays inside the plane row it belongs to.  No LDS, no scratch:
// every register array below is indexed with constants only.

struct PicReqK {
  const uint8_t *src[3];   // per plane: row 0 of the plane (bitstream order: the BOTTOM row of the picture)
  uint8_t *dst[3];
  int64_t dpitch[3];
  int spitch[3], pw[3], ph[3];   // source pitch, plane width / height in pixels (the full coded plane)
  int rx[3], ry[3], rw[3], rh[3];   // the rectangle per plane (display order: row 0 at the top); RGB formats use plane 0's
  int cpr[3];              // 16-pixel chunks per output row of each plane
  int unit_end[3];         // lanes of the request: plane p's units end at unit_end[p] (RGB formats: all of them in plane 0)
  int format, linear, hdec, vdec;
};
struct PicBatchK {
  PicReqK r[THIP_MAX_BATCH];
};

// bytes row[c .. c + 15] of a row of `rowbytes` bytes (a multiple of 8, the row 8-byte aligned); bytes at c + k >= rowbytes are
// unspecified
__device__ __forceinline__ uint4 pic_load16(const uint8_t *row, int c, int rowbytes) {
  const uint8_t *p = row + c;
  if ((((uintptr_t)p) & 15) == 0 && c + 16 <= rowbytes) return *reinterpret_cast<const uint4 *>(p);
  const uint32_t *rw = reinterpret_cast<const uint32_t *>(row);
  const int last = (rowbytes >> 2) - 1, d0 = c >> 2;
  uint32_t w[5];
#pragma unroll
  for (int k = 0; k < 5; k++) w[k] = rw[min(d0 + k, last)];
  const uint32_t sh = (uint32_t)(c & 3);
  uint4 r;
  r.x = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
  r.y = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
  r.z = __builtin_amdgcn_alignbyte(w[3], w[2], sh);
  r.w = __builtin_amdgcn_alignbyte(w[4], w[3], sh);
  return r;
}

__device__ __forceinline__ uint32_t pic_byte(const uint4 v, int j) {   // j: a constant after unrolling
  const uint32_t d = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
  return (d >> (8 * (j & 3))) & 255u;
}

// e[j] = chroma[b0 + j], j = 0..10, of one row of a horizontally decimated chroma plane of `cw` samples, the indices clamped
// to [0, cw - 1] (the edge of the full coded plane)
__device__ __forceinline__ void pic_chroma_window(const uint8_t *row, int b0, int cw, uint32_t e[11]) {
  const uint32_t *rw = reinterpret_cast<const uint32_t *>(row);
  const int last = (cw >> 2) - 1, d0 = b0 >> 2;   // (b0 >= -1: d0 >= -1; dword -1 only ever supplies position -1)
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = rw[max(0, min(d0 + k, last))];
  const uint32_t sh = (uint32_t)(b0 & 3);
  uint4 v;
  v.x = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
  v.y = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
  v.z = __builtin_amdgcn_alignbyte(w[3], w[2], sh);
  v.w = 0;
#pragma unroll
  for (int j = 0; j < 11; j++) e[j] = pic_byte(v, j);
  if (b0 < 0) e[0] = e[1];
  if (b0 + 11 > cw) {
    const uint32_t edge = row[cw - 1];
#pragma unroll
    for (int j = 0; j < 11; j++)
      if (b0 + j >= cw) e[j] = edge;
  }
}

// Chroma of the 16 pixels at luma columns c .. c + 15 (c & 1 == P) from a horizontally decimated plane: rows `ra` (the pixel's
// own chroma row) and `rn` (its vertical neighbour, read with VDEC only).  MODE 0 nearest, 1 linear along x, 2 linear along both.
template <int P, int MODE>
__device__ __forceinline__ void pic_chroma_dec(const uint8_t *ra, const uint8_t *rn, int c, int cw, uint32_t out[16]) {
  const int b0 = ((c - P) >> 1) - 1;   // window position 0 = the chroma column left of the first pixel's
  uint32_t ea[11];
  pic_chroma_window(ra, b0, cw, ea);
  if (MODE == 2) {
    uint32_t en[11];
    pic_chroma_window(rn, b0, cw, en);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int k = (P + i) >> 1, o = ((P + i) & 1) ? k + 2 : k;   // odd column: the right neighbour, even: the left one
      const uint32_t h0 = 3 * ea[1 + k] + ea[o], h1 = 3 * en[1 + k] + en[o];
      out[i] = (3 * h0 + h1 + 8) >> 4;   // = (9a + 3b + 3c + d + 8) >> 4
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int k = (P + i) >> 1, o = ((P + i) & 1) ? k + 2 : k;
      out[i] = MODE == 1 ? (3 * ea[1 + k] + ea[o] + 2) >> 2 : ea[1 + k];
    }
  }
}

// The library's integer Y'CbCr -> R'G'B' (include/theora_hip.h states it)
__device__ __forceinline__ uint32_t pic_clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }
__device__ __forceinline__ void pic_rgb(uint32_t Y, uint32_t Cb, uint32_t Cr, uint32_t &R, uint32_t &G, uint32_t &B) {
  const int y = 76309 * ((int)Y - 16) + 32768, u = (int)Cb - 128, v = (int)Cr - 128;
  R = pic_clamp255((y + 104597 * v) >> 16);
  G = pic_clamp255((y - 25675 * u - 53279 * v) >> 16);
  B = pic_clamp255((y + 132201 * u) >> 16);
}

__device__ __forceinline__ void pic_store_bytes(uint8_t *d, const uint32_t *w, int nbytes, int cap) {   // cap: a constant
#pragma unroll
  for (int b = 0; b < cap; b++)
    if (b < nbytes) d[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
}
// nwords (a constant, a multiple of 4) dwords to d: 16-byte stores for a whole chunk in an aligned row, bytes otherwise
template <int NW>
__device__ __forceinline__ void pic_store(uint8_t *d, const uint32_t *w, int nbytes) {
  if (nbytes == 4 * NW && (((uintptr_t)d) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < NW / 4; q++)
      reinterpret_cast<uint4 *>(d)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else {
    pic_store_bytes(d, w, nbytes, 4 * NW);
  }
}

__global__ __launch_bounds__(256) void k_picture_out(const PicBatchK B) {
  const PicReqK &R = B.r[blockIdx.y];
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);
  if (u >= R.unit_end[2]) return;
  if (R.format == THIP_PIC_YCBCR) {
    const int p = (u >= R.unit_end[0]) + (u >= R.unit_end[1]);
    const int v = u - (p ? R.unit_end[p - 1] : 0);
    const int j = v / R.cpr[p], k = v - j * R.cpr[p];
    const int c = R.rx[p] + 16 * k, n = min(16, R.rw[p] - 16 * k);
    const uint4 s = pic_load16(R.src[p] + (size_t)(R.ph[p] - 1 - (R.ry[p] + j)) * R.spitch[p], c, R.pw[p]);
    const uint32_t w[4] = {s.x, s.y, s.z, s.w};
    pic_store<4>(R.dst[p] + (size_t)j * R.dpitch[p] + 16 * k, w, n);
    return;
  }
  const int j = u / R.cpr[0], k = u - j * R.cpr[0];
  const int c = R.rx[0] + 16 * k, n = min(16, R.rw[0] - 16 * k);
  const int Yd = R.ry[0] + j;   // display row
  const uint4 ys = pic_load16(R.src[0] + (size_t)(R.ph[0] - 1 - Yd) * R.spitch[0], c, R.pw[0]);
  uint32_t cb[16], cr[16];
  if (!R.hdec) {   // 4:4:4: one chroma sample per pixel
    const size_t o1 = (size_t)(R.ph[1] - 1 - Yd) * R.spitch[1], o2 = (size_t)(R.ph[2] - 1 - Yd) * R.spitch[2];
    const uint4 bs = pic_load16(R.src[1] + o1, c, R.pw[1]), rs = pic_load16(R.src[2] + o2, c, R.pw[2]);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      cb[i] = pic_byte(bs, i);
      cr[i] = pic_byte(rs, i);
    }
  } else {
    const int ch = R.ph[1], cw = R.pw[1];
    const int cyd = Yd >> R.vdec;   // the pixel's chroma row; its vertical neighbour (4:2:0, linear): centred siting
    const int cyn = R.vdec ? min(max((Yd & 1) ? cyd + 1 : cyd - 1, 0), ch - 1) : cyd;
    const size_t oa = (size_t)(ch - 1 - cyd) * R.spitch[1], on = (size_t)(ch - 1 - cyn) * R.spitch[1];
    const int mode = R.linear ? (R.vdec ? 2 : 1) : 0;
    const bool odd = c & 1;
#define PIC_CHROMA(P_, M_)                                                        \
  do {                                                                            \
    pic_chroma_dec<P_, M_>(R.src[1] + oa, R.src[1] + on, c, cw, cb);              \
    pic_chroma_dec<P_, M_>(R.src[2] + oa, R.src[2] + on, c, cw, cr);              \
  } while (0)
    if (mode == 2) {
      if (odd) PIC_CHROMA(1, 2); else PIC_CHROMA(0, 2);
    } else if (mode == 1) {
      if (odd) PIC_CHROMA(1, 1); else PIC_CHROMA(0, 1);
    } else {
      if (odd) PIC_CHROMA(1, 0); else PIC_CHROMA(0, 0);
    }
#undef PIC_CHROMA
  }
  uint32_t r[16], g[16], b[16];
#pragma unroll
  for (int i = 0; i < 16; i++) pic_rgb(pic_byte(ys, i), cb[i], cr[i], r[i], g[i], b[i]);
  uint8_t *const d0 = R.dst[0] + (size_t)j * R.dpitch[0];
  if (R.format == THIP_PIC_RGBA32) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = r[i] | g[i] << 8 | b[i] << 16 | 0xFF000000u;
    pic_store<16>(d0 + 64 * k, w, 4 * n);
  } else if (R.format == THIP_PIC_RGB24) {
    uint32_t w[12];
#pragma unroll
    for (int q = 0; q < 12; q++) w[q] = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      w[(3 * i) >> 2] |= r[i] << (8 * ((3 * i) & 3));
      w[(3 * i + 1) >> 2] |= g[i] << (8 * ((3 * i + 1) & 3));
      w[(3 * i + 2) >> 2] |= b[i] << (8 * ((3 * i + 2) & 3));
    }
    pic_store<12>(d0 + 48 * k, w, 3 * n);
  } else {   // THIP_PIC_RGB_PLANAR
    uint32_t wr[4], wg[4], wb[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      wr[q] = r[4 * q] | r[4 * q + 1] << 8 | r[4 * q + 2] << 16 | r[4 * q + 3] << 24;
      wg[q] = g[4 * q] | g[4 * q + 1] << 8 | g[4 * q + 2] << 16 | g[4 * q + 3] << 24;
      wb[q] = b[4 * q] | b[4 * q + 1] << 8 | b[4 * q + 2] << 16 | b[4 * q + 3] << 24;
    }
    pic_store<4>(d0 + 16 * k, wr, n);
    pic_store<4>(R.dst[1] + (size_t)j * R.dpitch[1] + 16 * k, wg, n);
    pic_store<4>(R.dst[2] + (size_t)j * R.dpitch[2] + 16 * k, wb, n);
  }
}
