// k_picture_resize: a rectangle of a state's finished picture resampled to a caller-chosen size, converted and written to caller
// device memory as planar Y'CbCr, as 8-bit R'G'B' or as planar float R'G'B' (include/theora_hip.h, thip_picture_resize).  Included
// from thip_decode.hip behind thip_picture.h, whose pic_rgb, pic_byte and pic_store it uses.
//
// One lane makes 16 consecutive output samples of one output row, as in k_picture_out, and writes them with 16-byte stores where
// the destination row allows it.  Source samples are read one byte at a time: which bytes a sample needs depends on the scale, and
// every index is clamped to the request's rectangle, so no byte outside it is read.  The vertical position and weights are the
// same for all 16 samples; the horizontal position of the first is worked out once and stepped exactly after that (a quotient and
// a remainder of the step prepared on the host, added with a carry): no division per sample.  No LDS, no scratch: every register
// array below is indexed with constants only.

struct PicRszAxisK {   // one axis of one plane: source extent S, output extent O
  int S, O;
  int bq, br;          // bilinear: 256 S = bq O + br
  int aq, ar;          // area:         S = aq O + ar
};
struct PicRszReqK {
  const uint8_t *src[3];   // per plane: row 0 of the plane (bitstream order: the BOTTOM row of the picture)
  uint8_t *dst[3];
  int64_t dpitch[3];
  int spitch[3], ph[3];    // source pitch, plane height (the full coded plane)
  int rx[3], ry[3];        // the rectangle's corner per plane (display order: row 0 at the top)
  PicRszAxisK ax[3], ay[3];
  uint64_t area_d[3], area_m[3];   // area: D = S_x S_y; m != 0: floor(n / D) = mulhi64(n, m) for every n the kernel makes
  int cpr;                 // 16-sample chunks per output row of plane 0 (R'G'B': of the picture)
  int ccpr;                // ... of planes 1 and 2 (THIP_PIC_YCBCR)
  int unit_end[3];         // lanes of the request: plane p's units end at unit_end[p] (RGB formats: all of them in plane 0)
  int format, filter, elem;
  float scale[3], bias[3];
};
struct PicRszBatchK {
  PicRszReqK r[THIP_MAX_BATCH];
};

// The host's part: the steps of an axis, and the reciprocal of the area filter's divisor.
static inline void rsz_prepare_axis(PicRszAxisK &a, int S, int O) {
  a.S = S;
  a.O = O;
  a.bq = (int)(256 * (int64_t)S / O);
  a.br = (int)(256 * (int64_t)S % O);
  a.aq = S / O;
  a.ar = S % O;
}
// floor(n / D) = mulhi64(n, m) with m = floor(2^64 / D) + 1 for every n <= nmax = 255 D + (D >> 1) exactly when
// nmax (m D - 2^64) < 2^64 (what the excess of m adds to n / D then stays below 1 / D); otherwise, and for D = 1, m = 0: the
// kernel divides
static inline void rsz_prepare_area(PicRszReqK &K, int p, int sw, int sh) {
  const uint64_t D = (uint64_t)sw * (uint64_t)sh;
  K.area_d[p] = D;
  K.area_m[p] = 0;
  if (D < 2) return;
  const uint64_t m = ~(uint64_t)0 / D + 1;   // (D a power of two: m = 2^64 / D, the excess is 0 and every n is exact)
  const unsigned __int128 one = (unsigned __int128)1 << 64;
  const unsigned __int128 excess = (unsigned __int128)m * D - one, nmax = (unsigned __int128)255 * D + (D >> 1);
  if (excess * nmax < one) K.area_m[p] = m;
}

// floor((X * (q O + r) + c) / O) and the remainder, for 0 <= X < 2^14, 0 <= r < O <= 2^14 and |c| < 2^30: the 64-bit position
// X * step + c splits exactly into X q + floor((X r + c) / O), and X r + c fits 32 bits
__device__ __forceinline__ void rsz_start(int X, int q, int r, int c, int O, int &pq, int &pr) {
  const int t = X * r + c;
  int d = t / O, m = t - d * O;
  if (m < 0) {   // floor, not truncation
    m += O;
    d--;
  }
  pq = X * q + d;
  pr = m;
}
__device__ __forceinline__ void rsz_step(int q, int r, int O, int &pq, int &pr) {
  pq += q;
  pr += r;
  if (pr >= O) {
    pr -= O;
    pq++;
  }
}

// the source row `row` (display order inside the rectangle) of plane p, at the rectangle's first column
__device__ __forceinline__ const uint8_t *rsz_row(const PicRszReqK &R, int p, int row) {
  return R.src[p] + (size_t)(R.ph[p] - 1 - (R.ry[p] + row)) * R.spitch[p] + R.rx[p];
}

// THIP_FILTER_BILINEAR: out[i] = sample 16 k + i of output row j of plane p
__device__ __forceinline__ void rsz_bilinear16(const PicRszReqK &R, int p, int j, int k, uint32_t out[16]) {
  const PicRszAxisK &ax = R.ax[p], &ay = R.ay[p];
  int pq, pr;
  rsz_start(j, ay.bq, ay.br, 128 * (ay.S - ay.O), ay.O, pq, pr);
  const int py = min(max(pq, 0), (ay.S - 1) * 256);
  const int j0 = py >> 8, fy = py & 255, j1 = min(j0 + 1, ay.S - 1);
  const uint8_t *const r0 = rsz_row(R, p, j0), *const r1 = rsz_row(R, p, j1);
  rsz_start(16 * k, ax.bq, ax.br, 128 * (ax.S - ax.O), ax.O, pq, pr);
  const int xmax = (ax.S - 1) * 256;
#pragma unroll
  for (int i = 0; i < 16; i++) {   // (samples beyond the row's end clamp to its last position like any other)
    const int px = min(max(pq, 0), xmax);
    const int i0 = px >> 8, fx = px & 255, i1 = min(i0 + 1, ax.S - 1);
    const int a = r0[i0], b = r0[i1], c = r1[i0], d = r1[i1];
    out[i] = (uint32_t)((256 - fy) * ((256 - fx) * a + fx * b) + fy * ((256 - fx) * c + fx * d) + 32768) >> 16;
    rsz_step(ax.bq, ax.br, ax.O, pq, pr);
  }
}

// THIP_FILTER_AREA: output index X covers [X S, (X + 1) S) where source sample i covers [i O, (i + 1) O): it starts `off` units
// into sample `first` (X S = first O + off) and ends S units on, so measured from the start of `first` it is [off, off + S) and
// tap t, sample first + t, is [t O, (t + 1) O): the weight is the overlap of the two.  It reaches over ceil((off + S) / O) samples.
// The taps are the outer loop and the 16 samples the inner, unrolled one: 16 independent loads an iteration (a loop a sample
// would wait for one load at a time); a sample with fewer taps than the lane's most reads its clamped index with weight 0.
// n: the samples of the chunk that exist (the others are made too, from clamped indices, and never stored).
__device__ __forceinline__ void rsz_area16(const PicRszReqK &R, int p, int j, int k, int n, uint32_t out[16]) {
  const PicRszAxisK &ax = R.ax[p], &ay = R.ay[p];
  int first[16], off[16], taps = 0;
  {
    int pq, pr;
    rsz_start(16 * k, ax.aq, ax.ar, 0, ax.O, pq, pr);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      first[i] = pq;
      off[i] = pr;
      const int e = pr + ax.ar;   // off + S = aq O + e, 0 <= e < 2 O
      if (i < n) taps = max(taps, ax.aq + (e > 0) + (e > ax.O));
      rsz_step(ax.aq, ax.ar, ax.O, pq, pr);
    }
  }
  uint64_t acc[16];
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0;
  int row, offy;
  rsz_start(j, ay.aq, ay.ar, 0, ay.O, row, offy);
  int remy = ay.S, wy = min(ay.O - offy, remy);   // rows: the first takes what is left of its sample, then whole ones, then the rest
  while (remy > 0) {
    const uint8_t *const r = rsz_row(R, p, min(row, ay.S - 1));
    uint32_t sum[16];   // <= 255 S
#pragma unroll
    for (int i = 0; i < 16; i++) sum[i] = 0;
    for (int t = 0, b = 0; t < taps; t++, b += ax.O) {   // b = t O <= S + O
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int w = max(min(b + ax.O - off[i], ax.S) - max(b - off[i], 0), 0);
        sum[i] += (uint32_t)w * r[min(first[i] + t, ax.S - 1)];
      }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] += (uint64_t)(uint32_t)wy * sum[i];
    remy -= wy;
    row++;
    wy = min(ay.O, remy);
  }
  const uint64_t D = R.area_d[p], m = R.area_m[p], half = D >> 1;
#pragma unroll
  for (int i = 0; i < 16; i++) out[i] = (uint32_t)(m ? __umul64hi(acc[i] + half, m) : (acc[i] + half) / D);
}

__device__ __forceinline__ void rsz_plane16(const PicRszReqK &R, int p, int j, int k, int n, uint32_t out[16]) {
  if (R.filter == THIP_FILTER_AREA) rsz_area16(R, p, j, k, n, out);
  else rsz_bilinear16(R, p, j, k, out);
}

// (float)c * scale, rounded, then + bias, rounded: two binary32 operations.  Written as plain operators under contract(off): the
// runtime's __fmul_rn / __fadd_rn are plain operators too, compiled with contraction allowed, and once inlined the pair may be contracted into one fma.
__device__ __forceinline__ float rsz_norm(uint32_t c, float scale, float bias) {
#pragma clang fp contract(off)
  const float v = (float)c * scale;
  return v + bias;
}
#ifndef RSZ_F16_BITS   // binary32 -> binary16, round to nearest even (v_cvt_f16_f32)
#define RSZ_F16_BITS(v) ((uint32_t) __builtin_bit_cast(unsigned short, (_Float16)(v)))
#endif

// 16 components of one float plane: four 16-byte stores (F32) or two (F16) for a whole chunk in an aligned row
__device__ __forceinline__ void rsz_store_float(uint8_t *row, int k, int n, int elem, const uint32_t c[16], float scale, float bias) {
  if (elem == THIP_ELEM_F32) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = __builtin_bit_cast(uint32_t, rsz_norm(c[i], scale, bias));
    pic_store<16>(row + 64 * k, w, 4 * n);
  } else {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; q++)
      w[q] = RSZ_F16_BITS(rsz_norm(c[2 * q], scale, bias)) | RSZ_F16_BITS(rsz_norm(c[2 * q + 1], scale, bias)) << 16;
    pic_store<8>(row + 32 * k, w, 2 * n);
  }
}

__global__ __launch_bounds__(256) void k_picture_resize(const PicRszBatchK B) {
  const PicRszReqK &R = B.r[blockIdx.y];
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);
  if (u >= R.unit_end[2]) return;
  if (R.format == THIP_PIC_YCBCR) {
    const int p = (u >= R.unit_end[0]) + (u >= R.unit_end[1]);
    const int v = u - (p ? R.unit_end[p - 1] : 0), cpr = p ? R.ccpr : R.cpr;
    const int j = v / cpr, k = v - j * cpr;
    const int n = min(16, R.ax[p].O - 16 * k);
    uint32_t s[16];
    rsz_plane16(R, p, j, k, n, s);
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; q++) w[q] = s[4 * q] | s[4 * q + 1] << 8 | s[4 * q + 2] << 16 | s[4 * q + 3] << 24;
    pic_store<4>(R.dst[p] + (size_t)j * R.dpitch[p] + 16 * k, w, n);
    return;
  }
  const int j = u / R.cpr, k = u - j * R.cpr;
  const int n = min(16, R.ax[0].O - 16 * k);
  uint32_t r[16], g[16], b[16];
  {
    uint32_t ys[16], cb[16], cr[16];
    rsz_plane16(R, 0, j, k, n, ys);
    rsz_plane16(R, 1, j, k, n, cb);
    rsz_plane16(R, 2, j, k, n, cr);
#pragma unroll
    for (int i = 0; i < 16; i++) pic_rgb(ys[i], cb[i], cr[i], r[i], g[i], b[i]);
  }
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
  } else if (R.elem == THIP_ELEM_U8) {   // THIP_PIC_RGB_PLANAR
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
  } else {
    rsz_store_float(d0, k, n, R.elem, r, R.scale[0], R.bias[0]);
    rsz_store_float(R.dst[1] + (size_t)j * R.dpitch[1], k, n, R.elem, g, R.scale[1], R.bias[1]);
    rsz_store_float(R.dst[2] + (size_t)j * R.dpitch[2], k, n, R.elem, b, R.scale[2], R.bias[2]);
  }
}
