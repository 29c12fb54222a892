// k_picture_compare: a rectangle of a state's finished picture compared with a picture in caller device memory -- the exact sum
// of squared differences per plane and per 8x8 block, and the integer SSIM of include/theora_hip.h (thip_picture_compare).
// Included from thip_decode.hip.
//
// Everything is made from five sums over 4x4 cells counted from the rectangle's top-left: sx, sy, sxx, syy, sxy.  A cell's squared
// difference is sxx + syy - 2 sxy, an 8x8 block is 2x2 cells, an SSIM window is 2x2 cells at any cell position.  One lane owns 16
// columns of 8 rows, 4 x 2 cells: it reads each row of both pictures as four dwords (one 16-byte load a row where the 16 columns lie
// inside the rectangle and every row starts on 16 bytes, dwords where they start on 4, bytes elsewhere; samples outside the
// rectangle are never read and enter as 0 on both sides, which adds nothing to any sum) -- each lane chooses the path once for each
// of the two pictures, from its column count, its first row's address and the pitch, and the path has no branch inside, so the
// eight row loads of a side are in flight together; lanes at the right edge with fewer than 16 columns take the byte path and the
// wave runs both -- and forms the sums with v_dot4_u32_u8, four samples an
// instruction.  A work-group is 16 x 16 lanes, 256 columns of 128 rows.  Without SSIM every lane counts and nothing goes through
// LDS.  With SSIM the last lane column and lane row are the overlap: they load and sum like the others, but only to complete the
// windows that start in the 15 x 15 lanes before them; the next tile counts their samples.  Lanes pass the cells their left and
// upper neighbours need through LDS (a lane's upper cell row, and the first cell of its lower one), so no cell is summed twice
// inside a tile and a window costs four additions a sum plus two 64-bit divisions.  Sums are reduced in 32 bits (a tile's squared
// differences and its windows' Q20 values stay below 2^31): registers, the wave, the work-group, then one 64-bit integer
// atomic add per accumulator and work-group into the result, which the host zeroes on the stream before the launch.  Integer
// addition commutes, so the result does not depend on the order of arrival.  No scratch: every register array is indexed with
// constants only.

struct PicCmpReqK {
  const uint8_t *src[3];   // per plane: row 0 of the plane (bitstream order: the BOTTOM row of the picture)
  const uint8_t *ref[3];   // the other picture, rows top first
  int64_t rpitch[3];
  uint32_t *blk[3];        // block_sse, or NULL
  int64_t bpitch[3];
  thip_picture_metrics *res;
  int spitch[3], ph[3];    // source pitch, plane height (the full coded plane)
  int rx[3], ry[3], sw[3], sh[3];   // the rectangle per plane (display order: row 0 at the top)
  int tpr[3];              // tiles per tile row of each plane
  int tile_end[3];         // work-groups of the request: plane p's tiles end at tile_end[p]
  int flags;
};
struct PicCmpBatchK {
  PicCmpReqK r[THIP_MAX_BATCH];
};

#define CMP_C1 26634    // floor(64^2 (0.01 * 255)^2)
#define CMP_C2 239708   // floor(64^2 (0.03 * 255)^2)
#ifndef CMP_DOT4        // sum of the four byte products of a and b, plus c (v_dot4_u32_u8)
#define CMP_DOT4(a, b, c) __builtin_amdgcn_udot4((a), (b), (c), false)
#endif

// Columns [0, n) of rows [0, rows) of the 16 x 8 samples at p0 (row r at p0 + r * pitch; n in 1..16, rows in 1..8) as four dwords a
// row, byte k of a row in bits 8 (k & 3) of w[k >> 2]; samples outside are 0 and never read.  One decision for all eight rows, and
// no branch after it, so that the eight loads (bytes: 128) are in flight together: a row beyond `rows` reloads the last row there
// is and a column beyond n the last there is, and a select drops them.  16 columns whose rows all start on 16 bytes: one 16-byte
// load a row; on 4 bytes: four dwords; anything else: bytes.
__device__ __forceinline__ void cmp_load_rows(const uint8_t *p0, int64_t pitch, int n, int rows, uint32_t w[8][4]) {
  const uintptr_t al = ((uintptr_t)p0) | (uintptr_t)pitch;
  if (n >= 16 && (al & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint4 v = *reinterpret_cast<const uint4 *>(p0 + (int64_t)min(r, rows - 1) * pitch);
      const bool in = r < rows;
      w[r][0] = in ? v.x : 0u;
      w[r][1] = in ? v.y : 0u;
      w[r][2] = in ? v.z : 0u;
      w[r][3] = in ? v.w : 0u;
    }
  } else if (n >= 16 && (al & 3) == 0) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint32_t *row = reinterpret_cast<const uint32_t *>(p0 + (int64_t)min(r, rows - 1) * pitch);
#pragma unroll
      for (int q = 0; q < 4; q++) w[r][q] = r < rows ? row[q] : 0u;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint8_t *row = p0 + (int64_t)min(r, rows - 1) * pitch;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint32_t d = 0;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const uint32_t v = row[min(4 * q + t, n - 1)];
          d |= (4 * q + t < n && r < rows ? v : 0u) << (8 * t);
        }
        w[r][q] = d;
      }
    }
  }
}

// The five sums of the lane's 4 x 2 cells: columns x0 .. x0 + 15, rows y0 .. y0 + 7 of plane p's rectangle (cell 4 m + k: cell
// column k of cell row m).  S[0] = sx (the state's picture), S[1] = sy (ref), S[2] = sxx, S[3] = syy, S[4] = sxy.  A lane outside
// the rectangle reads nothing and returns zeros.
__device__ __forceinline__ void cmp_lane_cells(const PicCmpReqK &R, int p, int x0, int y0, uint32_t S[5][8]) {
#pragma unroll
  for (int q = 0; q < 5; q++)
#pragma unroll
    for (int c = 0; c < 8; c++) S[q][c] = 0;
  const int n = min(16, R.sw[p] - x0), rows = min(8, R.sh[p] - y0);
  if (n <= 0 || rows <= 0) return;
  uint32_t a[8][4], b[8][4];   // (the state's rows run upwards in memory: a negative pitch)
  cmp_load_rows(R.src[p] + (int64_t)(R.ph[p] - 1 - (R.ry[p] + y0)) * R.spitch[p] + R.rx[p] + x0, -(int64_t)R.spitch[p], n, rows, a);
  cmp_load_rows(R.ref[p] + (int64_t)y0 * R.rpitch[p] + x0, R.rpitch[p], n, rows, b);
#pragma unroll
  for (int r = 0; r < 8; r++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = 4 * (r >> 2) + k;
      S[0][c] = CMP_DOT4(a[r][k], 0x01010101u, S[0][c]);
      S[1][c] = CMP_DOT4(b[r][k], 0x01010101u, S[1][c]);
      S[2][c] = CMP_DOT4(a[r][k], a[r][k], S[2][c]);
      S[3][c] = CMP_DOT4(b[r][k], b[r][k], S[3][c]);
      S[4][c] = CMP_DOT4(a[r][k], b[r][k], S[4][c]);
    }
}

// w of one window from its five sums (include/theora_hip.h): |w| <= 2^20.  a, b and d are positive; c may be negative, and C's
// division rounds toward zero: the quotients are made from magnitudes and the sign put back.
__device__ __forceinline__ int32_t cmp_window_q20(uint32_t sx, uint32_t sy, uint32_t sxx, uint32_t syy, uint32_t sxy) {
  const int64_t xy = (int64_t)sx * sy, xx = (int64_t)sx * sx, yy = (int64_t)sy * sy;
  const int64_t a = 2 * xy + CMP_C1, b = xx + yy + CMP_C1;
  const int64_t c = 2 * (64 * (int64_t)sxy - xy) + CMP_C2, d = (64 * (int64_t)sxx - xx) + (64 * (int64_t)syy - yy) + CMP_C2;
  const uint64_t q1 = ((uint64_t)a << 20) / (uint64_t)b;
  const uint64_t q2 = ((uint64_t)(c < 0 ? -c : c) << 20) / (uint64_t)d;
  const int32_t w = (int32_t)((q1 * q2) >> 20);
  return c < 0 ? -w : w;
}

#ifdef __HIPCC__
__global__ __launch_bounds__(256) void k_picture_compare(const PicCmpBatchK B) {
  __shared__ uint32_t top[5][16][64];   // [sum][lane row][cell column of the tile]: the upper cell row of every lane
  __shared__ uint32_t low[5][16][16];   // [sum][lane row][lane column]: the first cell of every lane's lower cell row
  __shared__ uint32_t red[2][4];
  const PicCmpReqK &R = B.r[blockIdx.y];
  const int tile = (int)blockIdx.x;
  if (tile >= R.tile_end[2]) return;   // (the whole work-group)
  const int p = (tile >= R.tile_end[0]) + (tile >= R.tile_end[1]);
  const int v = tile - (p ? R.tile_end[p - 1] : 0);
  const int ty = v / R.tpr[p], tx = v - ty * R.tpr[p];
  const bool ssim = (R.flags & THIP_CMP_SSIM) != 0;
  const int T = ssim ? 15 : 16;   // lanes of the tile that count, per axis
  const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
  const int x0 = (tx * T + lx) * 16, y0 = (ty * T + ly) * 8;
  const int sw = R.sw[p], sh = R.sh[p];
  uint32_t S[5][8];
  cmp_lane_cells(R, p, x0, y0, S);
  const bool core = lx < T && ly < T;
  uint32_t sse = 0;
  int32_t wsum = 0;
  if (core) {
    uint32_t d[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
      d[c] = S[2][c] + S[3][c] - 2 * S[4][c];
      sse += d[c];
    }
    if (R.blk[p] && y0 < sh) {
      uint32_t *const row = R.blk[p] + (int64_t)(y0 >> 3) * R.bpitch[p] + (x0 >> 3);
      if (x0 < sw) row[0] = d[0] + d[1] + d[4] + d[5];
      if (x0 + 8 < sw) row[1] = d[2] + d[3] + d[6] + d[7];
    }
  }
  if (ssim) {
#pragma unroll
    for (int q = 0; q < 5; q++) {
      *reinterpret_cast<uint4 *>(&top[q][ly][4 * lx]) = make_uint4(S[q][0], S[q][1], S[q][2], S[q][3]);
      low[q][ly][lx] = S[q][4];
    }
    __syncthreads();
    // windows start at every cell of a counting lane; the last that fits starts at column sw - 8, row sh - 8
    if (core && x0 + 8 <= sw && y0 + 8 <= sh) {
      uint32_t H[5][3][4];   // cell (k, m) plus its right neighbour, cell rows m = 0..2 (2: the lane below's upper row)
#pragma unroll
      for (int q = 0; q < 5; q++) {
        const uint4 n = *reinterpret_cast<const uint4 *>(&top[q][ly + 1][4 * lx]);
        const uint32_t below[5] = {n.x, n.y, n.z, n.w, top[q][ly + 1][4 * lx + 4]};
        const uint32_t r0 = top[q][ly][4 * lx + 4], r1 = low[q][ly][lx + 1];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          H[q][0][k] = S[q][k] + (k < 3 ? S[q][(k + 1) & 3] : r0);
          H[q][1][k] = S[q][4 + k] + (k < 3 ? S[q][4 + ((k + 1) & 3)] : r1);
          H[q][2][k] = below[k] + below[k + 1];
        }
      }
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (x0 + 4 * k + 8 <= sw && y0 + 4 * m + 8 <= sh)
            wsum += cmp_window_q20(H[0][m][k] + H[0][m + 1][k], H[1][m][k] + H[1][m + 1][k], H[2][m][k] + H[2][m + 1][k],
                                   H[3][m][k] + H[3][m + 1][k], H[4][m][k] + H[4][m + 1][k]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sse += __shfl_down(sse, o);
    wsum += __shfl_down(wsum, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sse;
    red[1][threadIdx.x >> 6] = (uint32_t)wsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t e = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const int32_t w = (int32_t)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    if (R.flags & THIP_CMP_SSE) atomicAdd(reinterpret_cast<unsigned long long *>(&R.res->sse[p]), (unsigned long long)e);
    if (ssim) atomicAdd(reinterpret_cast<unsigned long long *>(&R.res->ssim_q20[p]), (unsigned long long)(long long)w);
    if (v == 0) {   // the counts are no sums: the plane's first tile states them
      if (R.flags & THIP_CMP_SSE) R.res->samples[p] = (int64_t)sw * sh;
      if (ssim) R.res->windows[p] = sw >= 8 && sh >= 8 ? (int64_t)(((sw - 8) >> 2) + 1) * (((sh - 8) >> 2) + 1) : 0;
    }
  }
}
#endif
