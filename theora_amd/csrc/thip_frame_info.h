// k_frame_info: the half of a frame that is not pixels -- which fragments were coded, from which reference, through which vector,
// with how many coefficients -- as maps and as a dense motion field in caller device memory (include/theora_hip.h,
// thip_frame_info_out), and k_frame_info_keep, which keeps a frame's command words for later requests (thip_state_set_frame_info).
// Included from thip_decode.hip behind thip_picture.h, whose pic_store it uses.
//
// The fragment maps are a gather: a lane per output fragment reads the fragment's word and writes its bytes.  The dense outputs
// are the memory-bound part (66 MB a 4K frame in float32): a lane makes 16 bytes of one output row -- four float32, eight float16
// or sixteen `valid` pixels -- and fetches the words of the luma fragments those pixels lie in once (two words, three for
// `valid`), not a word a pixel.  The 16-byte chunks of a row are counted from the 16-byte boundary at or below the row's first
// byte, so that every whole chunk is one aligned 16-byte store whatever the row's alignment (elements that are themselves
// misaligned go byte by byte); the partial chunks at a row's two ends are written byte by byte.  No LDS, no atomics, no scratch:
// every register array below is indexed with constants only.

#define THIP_FI_WORD_MASK 0xFFFF7F07u   // coded, refi, last_zzi and the vector: what the record keeps of a coded fragment's word0

struct FiReqK {
  const uint32_t *info;     // tiled: a frame's frag_info (two words a tile position, word0 is read); else the record: one word a fragment, raster
  uint8_t *kind[3], *ncoef[3], *mv[3];
  uint8_t *flow, *valid;
  int64_t kind_pitch[3], ncoef_pitch[3], mv_pitch[3], flow_pitch, valid_pitch;
  int nh[3], nv[3], fro[3], tiles_x[3], tile_off[3];
  int fc0[3], fr0[3], fw[3];   // the fragment rectangle per plane: first column, first row from the TOP, columns
  int x, y, w, h;           // the rectangle in luma pixels, display coordinates
  int cpr_flow, cpr_valid;  // lanes per row of the dense outputs: one more than the row's bytes / 16, rounded up (an unaligned row has two partial chunks)
  int unit_end[5];          // lanes of the request: fragment maps of planes 0..2, the field's two planes, `valid`
  int tiled, elem, refs;
};
struct FiBatchK {
  FiReqK r[THIP_MAX_BATCH];
};

// word0 of fragment (bx, by) of plane p; by counts from the BOTTOM (bitstream order)
__device__ __forceinline__ uint32_t fi_word(const FiReqK &R, int p, int bx, int by) {
  if (R.tiled) {   // what thip_state_frag_pos computes
    const int pos = (R.tile_off[p] + (by >> 2) * R.tiles_x[p] + (bx >> 4)) * THIP_TILE_FRAGS + ((bx >> 2) & 3) * 16 + hilb_inv(by & 3, bx & 3);
    return R.info[2 * (size_t)pos];
  }
  return R.info[(size_t)R.fro[p] + (size_t)by * R.nh[p] + bx];
}
// 0 uncoded, 1 intra, 2 coded from PREV, 3 coded from GOLD
__device__ __forceinline__ uint32_t fi_kind(uint32_t w) {
  const uint32_t refi = (w >> THIP_INFO_REFI_SHIFT) & 3u;
  return !(w & THIP_INFO_CODED) ? 0u : refi == THIP_FRAME_SELF ? 1u : refi == THIP_FRAME_PREV ? 2u : 3u;
}
// (vx, vy) = (mvx, -mvy), each as the byte the map holds; (0, 0) unless the fragment has a reference
__device__ __forceinline__ uint32_t fi_vx(uint32_t w, uint32_t kind) { return kind >= 2u ? (w >> THIP_INFO_MVX_SHIFT) & 255u : 0u; }
__device__ __forceinline__ uint32_t fi_vy(uint32_t w, uint32_t kind) { return kind >= 2u ? (0u - (w >> THIP_INFO_MVY_SHIFT)) & 255u : 0u; }

#ifndef FI_F16_BITS   // binary32 -> binary16 (v_cvt_f16_f32; every value here is exact)
#define FI_F16_BITS(v) ((uint32_t) __builtin_bit_cast(unsigned short, (_Float16)(v)))
#endif
// component c (0: vx / 2, 1: vy / 2) of a fragment's vector in pixels as the bits of the element type; 0 for a kind `refs` leaves out
__device__ __forceinline__ uint32_t fi_flow_bits(uint32_t w, int c, int refs, int elem) {
  const uint32_t kind = fi_kind(w);
  const bool on = (kind == 2u && (refs & THIP_FI_REF_PREV)) || (kind == 3u && (refs & THIP_FI_REF_GOLD));
  const int v = on ? (int)(int8_t)(c ? fi_vy(w, kind) : fi_vx(w, kind)) : 0;
  const float f = 0.5f * (float)v;
  return elem == THIP_ELEM_F32 ? __builtin_bit_cast(uint32_t, f) : FI_F16_BITS(f);
}

// Bytes [b0, b1) of a row of nb bytes that chunk k holds (elements of esz bytes, a power of two); false: none
__device__ __forceinline__ bool fi_chunk(const uint8_t *row, int nb, int esz, int k, int &b0, int &b1) {
  const int a = (int)(((uintptr_t)row) & 15);
  const int lead = (a & (esz - 1)) ? 0 : a;   // bytes between the 16-byte boundary the chunks count from and the row
  b0 = max(16 * k - lead, 0);
  b1 = min(16 * k - lead + 16, nb);
  return b0 < b1;
}

__device__ __forceinline__ void fi_maps(const FiReqK &R, int p, int v) {
  const int fr = v / R.fw[p], fc = v - fr * R.fw[p];
  const uint32_t w = fi_word(R, p, R.fc0[p] + fc, R.nv[p] - 1 - (R.fr0[p] + fr));
  const uint32_t kind = fi_kind(w);
  if (R.kind[p]) R.kind[p][(size_t)fr * R.kind_pitch[p] + fc] = (uint8_t)kind;
  if (R.ncoef[p]) R.ncoef[p][(size_t)fr * R.ncoef_pitch[p] + fc] = (uint8_t)(kind ? (w >> THIP_INFO_LAST_ZZI_SHIFT) & 127u : 0u);
  if (R.mv[p]) {
    uint8_t *const d = R.mv[p] + (size_t)fr * R.mv_pitch[p] + 2 * fc;
    d[0] = (uint8_t)fi_vx(w, kind);
    d[1] = (uint8_t)fi_vy(w, kind);
  }
}

// 16 bytes of row j of plane c of the field
__device__ __forceinline__ void fi_flow(const FiReqK &R, int c, int j, int k) {
  const int f32 = R.elem == THIP_ELEM_F32, esz = f32 ? 4 : 2;
  uint8_t *const row = R.flow + ((size_t)c * R.h + j) * R.flow_pitch;
  int b0, b1;
  if (!fi_chunk(row, R.w * esz, esz, k, b0, b1)) return;
  const int X0 = R.x + (f32 ? b0 >> 2 : b0 >> 1), c0 = X0 >> 3, by = R.nv[0] - 1 - ((R.y + j) >> 3);
  // at most eight pixels: two fragments
  const uint32_t e0 = fi_flow_bits(fi_word(R, 0, c0, by), c, R.refs, R.elem);
  const uint32_t e1 = fi_flow_bits(fi_word(R, 0, min(c0 + 1, R.nh[0] - 1), by), c, R.refs, R.elem);
  const int n1 = 8 * (c0 + 1) - X0;   // pixels of the chunk inside the first fragment (1..8)
  uint32_t o[4];
  if (f32) {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = i < n1 ? e0 : e1;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (2 * i < n1 ? e0 : e1) | (2 * i + 1 < n1 ? e0 : e1) << 16;
  }
  pic_store<4>(row + b0, o, b1 - b0);
}

// 16 bytes of row j of `valid`
__device__ __forceinline__ void fi_valid(const FiReqK &R, int j, int k) {
  uint8_t *const row = R.valid + (size_t)j * R.valid_pitch;
  int b0, b1;
  if (!fi_chunk(row, R.w, 1, k, b0, b1)) return;
  const int X0 = R.x + b0, c0 = X0 >> 3, by = R.nv[0] - 1 - ((R.y + j) >> 3), last = R.nh[0] - 1;
  // sixteen pixels: three fragments
  const uint32_t k0 = fi_kind(fi_word(R, 0, c0, by)), k1 = fi_kind(fi_word(R, 0, min(c0 + 1, last), by)),
                 k2 = fi_kind(fi_word(R, 0, min(c0 + 2, last), by));
  const int n1 = 8 * (c0 + 1) - X0;
  uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 16; i++) o[i >> 2] |= (i < n1 ? k0 : i < n1 + 8 ? k1 : k2) << (8 * (i & 3));
  pic_store<4>(row + b0, o, b1 - b0);
}

__global__ __launch_bounds__(256) void k_frame_info(const FiBatchK B) {
  const FiReqK &R = B.r[blockIdx.y];
  const int u = (int)(blockIdx.x * 256 + threadIdx.x);
  if (u >= R.unit_end[4]) return;
  if (u < R.unit_end[2]) {
    const int p = (u >= R.unit_end[0]) + (u >= R.unit_end[1]);
    fi_maps(R, p, u - (p ? R.unit_end[p - 1] : 0));
  } else if (u < R.unit_end[3]) {
    const int v = u - R.unit_end[2], r = v / R.cpr_flow, k = v - r * R.cpr_flow;   // r: row of [2][height]
    const int c = r >= R.h;
    fi_flow(R, c, r - (c ? R.h : 0), k);
  } else {
    const int v = u - R.unit_end[3], j = v / R.cpr_valid;
    fi_valid(R, j, v - j * R.cpr_valid);
  }
}

// The record (thip_state_set_frame_info): a lane per tile position reads the position's word0 -- consecutive lanes consecutive
// words, whether the frame's frag_info is device memory or the pinned staging buffer across PCIe -- and stores what k_frame_info
// needs of it at the fragment's raster index; positions outside the plane (ragged tiles) store nothing.
struct FiKeepK {
  const uint32_t *info;   // the frame's frag_info, tile order
  uint32_t *rec;          // nfrags words, fragment-index order
  int nh[3], nv[3], fro[3], tiles_x[3], tile_off[3];
  int npos;               // 64 * ntiles
};
__global__ __launch_bounds__(256) void k_frame_info_keep(const FiKeepK K) {
  const int pos = (int)(blockIdx.x * 256 + threadIdx.x);
  if (pos >= K.npos) return;
  const int tile = pos >> 6, lane = pos & 63;
  const int p = (tile >= K.tile_off[1]) + (tile >= K.tile_off[2]);
  const int t = tile - K.tile_off[p], ty = t / K.tiles_x[p], tx = t - ty * K.tiles_x[p];
  const int by = 4 * ty + hilb_row(lane & 15), bx = 16 * tx + 4 * (lane >> 4) + hilb_col(lane & 15);
  if (bx >= K.nh[p] || by >= K.nv[p]) return;
  const uint32_t w = K.info[2 * (size_t)pos];
  K.rec[(size_t)K.fro[p] + (size_t)by * K.nh[p] + bx] = (w & THIP_INFO_CODED) ? w & THIP_FI_WORD_MASK : 0u;
}
