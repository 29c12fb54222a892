// thip_encode.hip -- th_encode_* (include/theoraenc_hip.h): a Theora encoder, intra-only by default, with motion-compensated inter
// frames on request (TH_ENCCTL_THIP_SET_INTER_FRAMES).  The block work -- motion search, transform, quantiser, DC prediction, tokens
// and their stream order -- is the device stage of thip_encode.h and thip_encode_inter.h; the host merges the EOB runs, chooses the
// Huffman tables, the mode and vector codes and writes the bits.  With TH_ENCCTL_THIP_SET_DEVICE_PACK the token part of the packet
// (EOB runs, tables, bits) is made on the device too (thip_encode_pack.h) and the host writes the frame header only.  The bitstream
// is stated in the header comment of theoraenc_hip.h.
//
// What the bitstream fixes for encoder and decoder alike -- the tables, the frame's geometry (th_enc_ctx is a FrameGeometry), the
// quantisation matrix (the setup is a QuantParams: compute_qmat gives every step, and the setup header is written from it), the
// run-length and vector codes -- is thip_bitstream.h's, shared with the decoder's front end.
//
// The reference of an inter frame is the encoder's own reconstruction of the previous frame, made by a th_decode_* context of this
// library fed with every packet the encoder returns (loop filter included): the encoder's reference is then the decoder's picture by
// construction, bit for bit, and the decoder's kernels do the work (dequantisation, iDCT, prediction, the uncoded copies, the loop
// filter).  The price is a host round trip between frames: the packet must exist before the next frame's search can start.
//
// The rate controllers -- bitrate mode's, and two-pass with its pass file -- are host arithmetic in thip_ratectl.h (RateCtl, TwoPass),
// tested without a GPU.  This file keeps what touches the device (the probe's buffers, launches and read-back), hands the
// controllers the stream's facts by value (enc_stream), and times them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "../../include/theora_hip.h"
#include "../../include/theoraenc_hip.h"
#include "thip_device.h"
#include "thip_rate.h"
#include "thip_ratectl.h"
#include "thip_hufftrain.h"
#include "thip_quant.h"
#include "thip_encode_modes.h"
#include "thip_encode_bqi.h"
#include "thip_encode_mask.h"
#include "thip_encode_roi.h"
#include "thip_encode_rd.h"
#include "thip_encode_skip.h"
#include "thip_encode_rdq.h"
#include "thip_encode_pack.h"
#include "thip_encode_cut.h"
#include "thip_encode_entry.h"
#include "thip_bitstream.h"
#include "thip_ctx.h"
#include "thip_device_guard.h"

using namespace thip;

namespace {

#define ENC_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t e_ = (expr);                                                                                            \
    if (e_ != hipSuccess) {                                                                                            \
      fprintf(stderr, "theora_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__);        \
      return TH_EFAULT;                                                                                                \
    }                                                                                                                  \
  } while (0)

// MSB-first bit writer with a 64-bit accumulator
struct BitW {
  std::vector<uint8_t> *out;
  uint64_t acc = 0;
  int n = 0;   // bits in acc (< 8 after every put)
  void put(uint32_t v, int nb) {
    if (!nb) return;
    acc = acc << nb | (v & (nb == 32 ? 0xFFFFFFFFu : ((1u << nb) - 1)));
    n += nb;
    while (n >= 8) {
      n -= 8;
      out->push_back((uint8_t)(acc >> n));
    }
  }
  void flush() {
    if (n) out->push_back((uint8_t)(acc << (8 - n)));
    n = 0;
    acc = 0;
  }
};

// ---- the setup header's contents (theoraenc_hip.h) -------------------------------------------------------------------
struct EncSetup {
  QuantParams qp;               // built in: three base matrices (luma intra, chroma intra, inter); one range of 63 a (qti, pli), both
                                // ends alike.  A caller's (TH_ENCCTL_SET_QUANT_PARAMS): consolidated, as the header carries them
  bool custom_quant = false;    // qp is a caller's: the header's quantiser part is then libtheora's packing (thip_quant.h)
  QuantCopy quant;              // qp as a th_quant_info, what TH_ENCCTL_THIP_GET_QUANT_PARAMS hands out
  uint32_t code[80][32];        // Huffman codes (MSB first), lengths
  uint8_t len[80][32];
  std::vector<uint8_t> trees;   // the 80 trees as written (spec 6.4.4), a bit string packed MSB first ...
  int64_t tree_bits;            // ... of this many bits
};

// the token weights of Huffman group hg, table t (theoraenc_hip.h): sparsity s, magnitude ratio q
void enc_token_weights(int hg, int t, double w[32]) {
  static const double kS[4] = {0.1, 0.3, 0.55, 0.8}, kQ[4] = {0.15, 0.35, 0.55, 0.75};
  const double s = kS[t & 3], q = kQ[t >> 2], e = 0.3 + 0.6 * s;
  for (int k = 0; k < 6; k++) w[k] = s * pow(e, k);                       // EOB runs 1, 2, 3, 4-7, 8-15, 16-31
  w[6] = s * pow(e, hg == 0 ? 3 : 5);                                      // 32-4095
  w[7] = (1 - s) * s * 0.5;                                                // SHORT_ZRL
  w[8] = (1 - s) * s * s * 0.3;                                            // ZRL
  w[9] = w[10] = (1 - s) * 0.5;                                            // +-1
  w[11] = w[12] = (1 - s) * 0.5 * q;                                       // +-2
  for (int k = 13; k <= 16; k++) w[k] = (1 - s) * pow(q, 2 + 0.5 * (k - 13));   // +-3 .. +-6
  for (int k = 17; k <= 22; k++) w[k] = (1 - s) * pow(q, k - 13);          // 7-8, 9-12, 13-20, 21-36, 37-68, 69-580
  for (int g = 1; g <= 5; g++) w[22 + g] = (1 - s) * 0.5 * pow(s, g);      // RUN_CAT1A
  w[28] = (1 - s) * pow(s, 6) * 2;                                         // RUN_CAT1B
  w[29] = (1 - s) * pow(s, 10) * 4;                                        // RUN_CAT1C
  w[30] = (1 - s) * s * q;                                                 // RUN_CAT2A
  w[31] = (1 - s) * s * s * q;                                             // RUN_CAT2B
}

// the setup's codes and lengths from a valid code set, and the 80 trees as the header writes them (thip_hufftrain.h)
void enc_setup_codes(EncSetup &s, const th_huff_code codes[80][32]) {
  s.trees.clear();
  BitW t{&s.trees};
  for (int h = 0; h < 80; h++) {
    for (int tok = 0; tok < 32; tok++) {
      s.len[h][tok] = (uint8_t)codes[h][tok].nbits;
      s.code[h][tok] = (uint32_t)((uint64_t)codes[h][tok].pattern & (((uint64_t)1 << codes[h][tok].nbits) - 1));
    }
    huff_tree_write(codes[h], [&](uint32_t v, int nb) { t.put(v, nb); });
  }
  s.tree_bits = (int64_t)s.trees.size() * 8 + t.n;
  t.flush();
}

// the built-in codes: the Huffman code (thip_hufftrain.h, huff_build) of enc_token_weights in 40-bit fixed point
void enc_builtin_codes(th_huff_code codes[80][32]) {
  for (int h = 0; h < 80; h++) {
    double w[32];
    uint64_t wi[32];
    uint32_t code[32];
    uint8_t len[32];
    enc_token_weights(h >> 4, h & 15, w);
    for (int k = 0; k < 32; k++) wi[k] = 1 + (uint64_t)(w[k] * (double)(1ull << 40));
    huff_build(wi, code, len);
    for (int k = 0; k < 32; k++) codes[h][k] = th_huff_code{code[k], (int)len[k]};
  }
}

// the built-in quantisation parameters (theoraenc_hip.h, "Setup header")
void enc_setup_builtin_quant(EncSetup &s) {
  QuantParams &q = s.qp;
  for (int qi = 0; qi < 64; qi++) {
    q.lflims[qi] = (uint8_t)((31 * (63 - qi) + 31) / 63);
    q.acscale[qi] = (uint16_t)lround(400.0 * pow(10.0 / 400.0, qi / 63.0));
    q.dcscale[qi] = (uint16_t)lround(200.0 * pow(10.0 / 200.0, qi / 63.0));
  }
  q.nbms = 3;
  q.bms.resize(3 * 64);
  for (int r = 0; r < 8; r++)
    for (int c = 0; c < 8; c++) {
      q.bms[0 * 64 + r * 8 + c] = (uint8_t)(16 + 3 * (r + c) + (r * c) / 4);
      q.bms[1 * 64 + r * 8 + c] = (uint8_t)(18 + 5 * (r + c));
      q.bms[2 * 64 + r * 8 + c] = (uint8_t)(16 + 2 * (r + c));
    }
  for (int qti = 0; qti < 2; qti++)
    for (int pli = 0; pli < 3; pli++) {
      q.nqrs[qti][pli] = 1;
      q.qrsizes[qti][pli][0] = 63;
      q.qrbmis[qti][pli][0] = q.qrbmis[qti][pli][1] = qti ? 2 : pli ? 1 : 0;
    }
  s.custom_quant = false;
  s.quant.assign(q);
}

void enc_setup_init(EncSetup &s) {
  enc_setup_builtin_quant(s);
  std::vector<th_huff_code> codes(80 * 32);
  enc_builtin_codes((th_huff_code(*)[32])codes.data());
  enc_setup_codes(s, (const th_huff_code(*)[32])codes.data());
}

// spec 7.2.1 (long: runs up to 4129, a new bit after a run of 4129) and 7.2.2 (short: runs up to 30, the bit always flips; the
// block flags of partially coded super blocks never hold a longer run, since each such super block has a block of either value)
void enc_put_runs(BitW &bw, const std::vector<uint8_t> &bits, bool lng) {
  const RunCode &rc = lng ? kLongRuns : kShortRuns;
  const size_t n = bits.size(), maxrun = (size_t)rc.longest();
  if (!n) return;
  int cur = bits[0];
  bw.put((uint32_t)cur, 1);
  size_t i = 0;
  while (i < n) {
    size_t j = i;
    while (j < n && bits[j] == cur && j - i < maxrun) j++;
    const int run = (int)(j - i);
    int k = 0;
    while (run >= rc.cls[k].start + (1 << rc.cls[k].bits)) k++;
    if (k < rc.last) bw.put((2u << k) - 2, k + 1);   // k ones and a zero
    else bw.put((1u << k) - 1, k);                   // the last class: all ones
    bw.put((uint32_t)(run - rc.cls[k].start), rc.cls[k].bits);
    i = j;
    if (i >= n) break;
    if (lng && (size_t)run == maxrun) {
      cur = bits[i];
      bw.put((uint32_t)cur, 1);
    } else {
      cur ^= 1;
    }
  }
}

// spec 7.5.1: one vector component written in scheme mvs (0: the VLC of Table 7.23)
void enc_put_mv(BitW &bw, int v, int mvs) {
  if (mvs) {
    bw.put((uint32_t)abs(v), 5);
    bw.put(v < 0, 1);
  } else {
    bw.put(kMvVlc.code[v + 31], kMvVlc.nbits[v + 31]);
  }
}

}  // namespace

constexpr size_t kEncPackRecBytes = sizeof(PackRec) + 320 * 4;   // d_prec / h_prec: the packetiser's record, then its histogram
constexpr int kEncSmallMask = 194;   // d_small / h_small: the word at which a masked frame's MaskRec lies (8-byte aligned)
constexpr int kEncSmallRoi = 198;    // ... and a frame's with a region-of-interest map its RoiRec (behind the MaskRec)

struct th_enc_ctx : thip_ctx_head, FrameGeometry {   // (the geometry: thip_bitstream.h)
  int device_req, device = -1;
  bool dev_ready = false;
  int cx0[3], cy0[3], cw[3], ch[3];   // the picture region per plane (spec 4.4), rows from the top
  EncSetup setup;
  int qi;
  int nheaders_out = 0;
  std::vector<uint8_t> hdr;
  int64_t packetno = 0;
  // frames: the one queued on the device, duplicates to follow it, frame counters (3.2.1 granule numbering)
  bool frame_pending = false, done = false;
  int dup_next = 0, dups_left = 0;
  int64_t cur = -1, key = -1;
  int frame_qi = 0;
  // device state
  hipStream_t stream = nullptr;
  hipEvent_t ev_in = nullptr, ev_read = nullptr, ev_t0 = nullptr, ev_done = nullptr;
  uint8_t *d_pix = nullptr, *h_pix = nullptr;   // host input: the three picture planes, packed
  uint8_t *d_rgb = nullptr, *h_rgb = nullptr;   // TH_ENCCTL_THIP_RGB_IN from host memory: the picture's rows, packed (4 bytes a pixel)
  hipEvent_t ev_conv = nullptr;                 // ... from device memory: the conversion has read the caller's picture
  // quality statistics (TH_ENCCTL_THIP_SET_QUALITY_STATS): the metrics of the last packet, made on the device and copied to h_qm
  int qflags = 0;
  bool q_queued = false;
  thip_picture_metrics *d_qm = nullptr, *h_qm = nullptr;
  hipEvent_t ev_m0 = nullptr, ev_m1 = nullptr;
  thip_enc_quality_stats qstats{};
  size_t pix_off[3], pix_bytes = 0;
  int32_t *d_order = nullptr;
  uint16_t *d_dequant = nullptr;                // [64 qi][3][64]
  int16_t *d_levels = nullptr, *d_dcq = nullptr;
  uint32_t *d_tok = nullptr, *d_cnt = nullptr, *d_base = nullptr, *d_small = nullptr, *d_out = nullptr;
  uint64_t *d_mask = nullptr;
  uint32_t *h_small = nullptr;                  // list lengths [3][64], overflow; with activity masking its record at kEncSmallMask
  uint32_t *h_tok = nullptr;
  size_t h_tok_cap = 0;
  int nchunks = 0;
  // inter frames (TH_ENCCTL_THIP_SET_INTER_FRAMES)
  bool inter = false, frame_key = true;
  int64_t kf_interval = 1;
  int nmbx = 0, nmbs = 0;
  int lambda[64];                  // the search's weight at each qi: the inter step of zig-zag index 1
  uint32_t *d_mb = nullptr, *d_dclast = nullptr, *h_mb = nullptr;
  uint8_t *d_cmap = nullptr, *h_cmap = nullptr;
  int16_t *d_dcr = nullptr;
  uint16_t *d_dqi = nullptr;       // [64 qi][intra, inter][3][64]
  th_dec_ctx *dec = nullptr;       // the reconstruction: a decoder of the encoder's own packets
  bool have_recon = false;
  thip_enc_inter_stats istats;
  // all eight modes (TH_ENCCTL_THIP_SET_INTER_MODES): k_enc_me_all's words a macro block
  bool modes = false;
  uint4 *d_mb4 = nullptr, *h_mb4 = nullptr;
  thip_enc_mode_stats mstats;
  // block-level qi (TH_ENCCTL_THIP_SET_BLOCK_QI): the delta (0 off), the frame's qi list, one qii a block (coded order)
  int bqi = 0, fnqis = 1, fqis[3] = {0, 0, 0};
  int bqi_hti[2][2] = {{5, 5}, {5, 5}};   // AC luma, AC chroma tables of the last packet of each type (key, inter)
  uint8_t *d_qii = nullptr, *h_qii = nullptr, *d_bqbits = nullptr;
  thip_enc_block_qi_stats bstats;
  // activity masking (TH_ENCCTL_THIP_SET_MASKING; thip_encode_mask.h): the ratio k (0 off); the frame queued has its scales in d_iscale
  int mask = 0;
  bool mask_queued = false;
  uint32_t *d_act = nullptr;
  MaskPart *d_mpart = nullptr;
  uint16_t *d_iscale = nullptr;
  hipEvent_t ev_a0 = nullptr, ev_a1 = nullptr;
  thip_enc_mask_stats kstats;
  // region of interest (TH_ENCCTL_THIP_SET_ROI_MAP; thip_encode_roi.h): the encoder's copy of the map in force (roi_on), tight rows;
  // the frame queued has its scales, on top of masking's, in d_iscale (roi_queued)
  bool roi_on = false, roi_queued = false;
  int roi_w = 0, roi_h = 0;
  size_t roi_cap = 0;            // bytes of d_roimap
  int8_t *d_roimap = nullptr;
  uint32_t *d_roiclamp = nullptr;   // what the copy of a device map clamped
  RoiPart *d_roipart = nullptr;
  hipEvent_t ev_o0 = nullptr, ev_o1 = nullptr;
  thip_enc_roi_stats ostats;
  // the rate-distortion mode decision (TH_ENCCTL_THIP_SET_RD_MODES; thip_encode_rd.h): the frame queued was decided by it (rd_queued)
  // with lambda rd_lam and the tables rd_used; rd_hti: DC luma, DC chroma, AC luma, AC chroma of the last inter packet
  bool rd = false, rd_queued = false;
  int rd_hti[4] = {5, 5, 5, 5}, rd_used[4] = {0, 0, 0, 0};
  int64_t rd_lam = 0;
  uint4 *d_cand = nullptr;
  uint8_t *d_rdbits = nullptr;   // [16 tables][5 Huffman groups][32 tokens]: code length + extra bits
  hipEvent_t ev_r0 = nullptr, ev_r1 = nullptr;
  thip_enc_rd_stats dstats;
  // the skip decision (TH_ENCCTL_THIP_SET_RD_SKIP; thip_encode_skip.h): the frame queued was decided by it (skip_queued) with the
  // unscaled lambda skip_lam; one flag a fragment (raster) where the test left a block uncoded
  bool skip = false, skip_queued = false;
  int64_t skip_lam = 0;
  uint8_t *d_skf = nullptr, *h_skf = nullptr;
  hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr;
  thip_enc_skip_stats sstats;
  // the level choice (TH_ENCCTL_THIP_SET_RD_QUANT; thip_encode_rdq.h): its weight (0: off); the frame queued went through it
  // (rdq_queued) with the unscaled lambda rdq_lam; the frame's sums (RdqOut::sums) on the device and where they are read back
  int rdq = 0;
  bool rdq_queued = false;
  int64_t rdq_lam = 0;
  unsigned long long *d_rdqsums = nullptr, *h_rdqsums = nullptr;
  hipEvent_t ev_z0 = nullptr, ev_z1 = nullptr;
  thip_enc_rd_quant_stats zstats;
  // bitrate mode (TH_ENCCTL_SET_BITRATE): the controller (thip_ratectl.h) and the probe's device state
  bool rate = false, rate_dropped = false, rate_dev = false;
  RateCtl ratectl;
  int rate_nwg = 0;
  int16_t *d_coef = nullptr, *d_qdc = nullptr;
  uint64_t *d_rcoded = nullptr, *d_rcls = nullptr;
  uint4 *d_rmbs = nullptr;
  uint2 *d_rtab = nullptr;
  int *d_rlam = nullptr;
  uint8_t *d_rlens = nullptr;
  uint32_t *d_rpart = nullptr;
  int64_t *d_rest = nullptr, *h_rest = nullptr;
  hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;
  // the device packetiser (TH_ENCCTL_THIP_SET_DEVICE_PACK; thip_encode_pack.h): on from the next frame; queued for the frame pending
  bool dpack = false, frame_dpack = false;
  int pack_groups = 0, pack_fallbacks = 0;
  size_t pack_cap = 0, h_pk_cap = 0;   // bytes of d_pk, h_pk
  uint8_t *d_pk = nullptr, *h_pk = nullptr;
  uint32_t *d_pglast = nullptr, *d_phist = nullptr, *d_pcodes = nullptr, *d_pcl = nullptr;
  PackSum *d_pgsum = nullptr, *d_pgbase = nullptr;
  PackRec *d_prec = nullptr, *h_prec = nullptr;
  hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr, ev_q0 = nullptr, ev_q1 = nullptr;
  thip_enc_pack_stats pstats;
  // automatic key frames (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES; thip_encode_cut.h): the ratio t (0 off); the measurement of the frame
  // queued (cnext) becomes the last packet's (cstats) in th_encode_packetout
  int auto_kf = 0;
  CutSums *d_cut = nullptr, *h_cut = nullptr;
  hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;
  thip_enc_cut_stats cnext, cstats;
  // two-pass (TH_ENCCTL_THIP_2PASS_OUT / _IN): the pass file and the second controller (thip_ratectl.h)
  TwoPass twopass;
  bool probe_queued = false;   // pass 1, quality mode: the frame queued has its probe in flight (read in packetout)
  // output: pkt_data is pkt's (the host packer, empty packets) or h_pk (the device packetiser)
  const uint8_t *pkt_data = nullptr;
  size_t pkt_size = 0;
  std::vector<uint8_t> pkt;
  std::vector<uint32_t> merged;
  thip_enc_frame_stats stats;
  thip_enc_token_hist thist;   // TH_ENCCTL_THIP_GET_TOKEN_HIST: the last packet's
  double device_ms = 0, host_ms = 0;
};

extern "C" {

// lambda[qi], the weight of every decision made at qi: the inter luma step at zig-zag index 1 of the parameters in force
static void enc_setup_lambda(th_enc_ctx *e) {
  for (int qi = 0; qi < 64; qi++) {
    uint16_t step[64];
    compute_qmat(e->setup.qp, 1, 0, qi, step);
    e->lambda[qi] = step[1];
  }
}

th_enc_ctx *th_encode_alloc_on(const th_info *info, int device) {
  if (!info) return nullptr;
  const th_info &i = *info;
  if (!i.frame_width || !i.frame_height || (i.frame_width & 15) || (i.frame_height & 15) || i.frame_width >= (1u << 20) ||
      i.frame_height >= (1u << 20))
    return nullptr;
  // (the frame's sides are below 1 << 20: an unsigned field too large for an int is a negative one, which the rule refuses as well)
  const PicRect pic{(int)i.pic_x, (int)i.pic_y, (int)i.pic_width, (int)i.pic_height};
  if (pic_outside(pic, (int)i.frame_width, (int)i.frame_height) || i.pic_x > 255 || i.frame_height - i.pic_height - i.pic_y > 255)
    return nullptr;
  if ((int)i.pixel_fmt < 0 || (int)i.pixel_fmt >= TH_PF_NFORMATS || i.pixel_fmt == TH_PF_RSVD) return nullptr;
  if (i.quality < 0 || i.quality > 63 || i.keyframe_granule_shift < 0 || i.keyframe_granule_shift > 31) return nullptr;
  if (i.target_bitrate != 0) return nullptr;   // bitrate mode needs rate control
  if (!i.fps_numerator || !i.fps_denominator || i.aspect_numerator >= (1u << 24) || i.aspect_denominator >= (1u << 24) ||
      (int)i.colorspace < 0 || (int)i.colorspace >= TH_CS_NSPACES)
    return nullptr;
  th_enc_ctx *e = new (std::nothrow) th_enc_ctx();
  if (!e) return nullptr;
  e->info = i;
  e->info.version_major = 3;
  e->info.version_minor = 2;
  e->info.version_subminor = 1;
  e->granpos_bias = 1;
  e->device_req = device;
  e->qi = i.quality;
  build_geometry(*e, (int)i.frame_width, (int)i.frame_height, (int)i.pixel_fmt);
  for (int p = 0; p < 3; p++) {
    const PicSpan sx = pic_span(pic.x, pic.w, p ? e->hdec : 0), sy = pic_span(pic.y, pic.h, p ? e->vdec : 0);
    e->cx0[p] = sx.x0;
    e->cy0[p] = sy.x0;
    e->cw[p] = sx.n;
    e->ch[p] = sy.n;
  }
  e->nmbx = e->nh[0] >> 1;
  e->nmbs = (int)e->mbs.size();
  e->nchunks = (e->nfrags + kEncChunk - 1) / kEncChunk;
  enc_setup_init(e->setup);
  enc_setup_lambda(e);
  memset(&e->stats, 0, sizeof(e->stats));
  memset(&e->thist, 0, sizeof(e->thist));
  memset(&e->istats, 0, sizeof(e->istats));
  memset(&e->mstats, 0, sizeof(e->mstats));
  memset(&e->bstats, 0, sizeof(e->bstats));
  memset(&e->kstats, 0, sizeof(e->kstats));
  memset(&e->ostats, 0, sizeof(e->ostats));
  memset(&e->dstats, 0, sizeof(e->dstats));
  memset(&e->sstats, 0, sizeof(e->sstats));
  memset(&e->zstats, 0, sizeof(e->zstats));
  memset(&e->pstats, 0, sizeof(e->pstats));
  memset(&e->cnext, 0, sizeof(e->cnext));
  memset(&e->cstats, 0, sizeof(e->cstats));
  e->dpack =thip_option("enc_device_pack") != 0;
  e->kf_interval = (int64_t)1 << i.keyframe_granule_shift;
  return e;
}

th_enc_ctx *th_encode_alloc(const th_info *info) { return th_encode_alloc_on(info, -1); }

// frees whatever device state exists (also a partial one, after a failed enc_ensure_device) and forgets it
static void enc_free_device(th_enc_ctx *e) {
  if (e->device < 0) return;
  DeviceGuard g(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->dec) th_decode_free(e->dec);
  e->dec = nullptr;
  e->have_recon = false;
  // one line a feature, in the order of th_enc_ctx, with the function that allocates it: a new buffer goes into that function and
  // its line here
  void **dev[] = {
      (void **)&e->d_pix, (void **)&e->d_order, (void **)&e->d_dequant, (void **)&e->d_levels, (void **)&e->d_dcq, (void **)&e->d_tok,
      (void **)&e->d_cnt, (void **)&e->d_base, (void **)&e->d_small, (void **)&e->d_out, (void **)&e->d_mask,   // enc_alloc_device
      (void **)&e->d_mb, (void **)&e->d_dclast, (void **)&e->d_cmap, (void **)&e->d_dcr, (void **)&e->d_dqi,       // ... inter frames
      (void **)&e->d_mb4,                                                                                            // enc_modes_alloc
      (void **)&e->d_qii, (void **)&e->d_bqbits,                                                                     // enc_bqi_prepare
      (void **)&e->d_act, (void **)&e->d_mpart, (void **)&e->d_iscale,                                               // enc_mask_queue
      (void **)&e->d_roimap, (void **)&e->d_roiclamp, (void **)&e->d_roipart,                                        // enc_roi_set, enc_roi_queue
      (void **)&e->d_cand, (void **)&e->d_rdbits,                                                                    // enc_rd_queue
      (void **)&e->d_skf,                                                                                            // enc_skip_queue
      (void **)&e->d_rdqsums,                                                                                        // enc_rdq_queue
      (void **)&e->d_coef, (void **)&e->d_qdc, (void **)&e->d_rcoded, (void **)&e->d_rcls, (void **)&e->d_rmbs, (void **)&e->d_rtab,
      (void **)&e->d_rlam, (void **)&e->d_rlens, (void **)&e->d_rpart, (void **)&e->d_rest,                         // enc_rate_alloc
      (void **)&e->d_pk, (void **)&e->d_pglast, (void **)&e->d_pcodes, (void **)&e->d_pcl, (void **)&e->d_pgsum,
      (void **)&e->d_pgbase, (void **)&e->d_prec,                                                                    // enc_pack_alloc
      (void **)&e->d_cut,                                                                                            // enc_cut_alloc
      (void **)&e->d_rgb,                                                                                            // enc_rgb_in
      (void **)&e->d_qm};                                                                                            // enc_quality_queue
  for (void **p : dev) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  void **host[] = {(void **)&e->h_pix, (void **)&e->h_small, (void **)&e->h_tok,   // enc_alloc_device
                   (void **)&e->h_mb, (void **)&e->h_cmap,                        // ... inter frames
                   (void **)&e->h_mb4,                                            // enc_modes_alloc
                   (void **)&e->h_qii,                                            // enc_bqi_prepare
                   (void **)&e->h_skf,                                            // enc_skip_queue
                   (void **)&e->h_rdqsums,                                        // enc_rdq_queue
                   (void **)&e->h_rest,                                           // enc_rate_alloc
                   (void **)&e->h_pk, (void **)&e->h_prec,                        // enc_pack_alloc
                   (void **)&e->h_cut,                                            // enc_cut_alloc
                   (void **)&e->h_rgb,                                            // enc_rgb_in
                   (void **)&e->h_qm};                                            // enc_quality_queue
  for (void **p : host) {
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
  }
  e->d_phist = nullptr;   // (it lay in d_prec's allocation)
  e->h_tok_cap = e->h_pk_cap = e->pack_cap = 0;
  e->pkt_data = nullptr;   // (it may have been h_pk)
  e->pkt_size = 0;
  e->rate_dev = false;
  e->q_queued = false;
  e->mask_queued = false;
  e->roi_on = e->roi_queued = false;   // (the map went with the buffers)
  e->roi_cap = 0;
  e->ostats.active = 0;
  e->rd_queued = false;
  e->skip_queued = false;
  e->rdq_queued = false;
  e->probe_queued = false;
  for (hipEvent_t *ev : {&e->ev_in, &e->ev_read, &e->ev_t0, &e->ev_done, &e->ev_p0, &e->ev_p1, &e->ev_k0, &e->ev_k1, &e->ev_q0, &e->ev_q1,
                          &e->ev_c0, &e->ev_c1, &e->ev_conv, &e->ev_m0, &e->ev_m1, &e->ev_a0, &e->ev_a1, &e->ev_r0, &e->ev_r1, &e->ev_s0, &e->ev_s1,
                          &e->ev_z0, &e->ev_z1, &e->ev_o0, &e->ev_o1}) {
    if (*ev) (void)hipEventDestroy(*ev);
    *ev = nullptr;
  }
  if (e->stream) (void)hipStreamDestroy(e->stream);
  e->stream = nullptr;
  e->dev_ready = false;
}

void th_encode_free(th_enc_ctx *e) {
  if (!e) return;
  enc_free_device(e);
  delete e;
}

static int enc_alloc_device(th_enc_ctx *e);

// everything on the device, at the first frame: worst-case buffers (kEncTokWords words a block)
static int enc_ensure_device(th_enc_ctx *e) {
  if (e->dev_ready) return 0;
  int dev = e->device_req;
  if (dev < 0) {
    const int opt = thip_option("device");
    if (opt == -2) {
      static std::atomic<unsigned> next{0};
      const int n = thip_device_count();
      dev = n > 0 ? (int)(next.fetch_add(1) % (unsigned)n) : -1;
    } else if (opt >= 0) {
      dev = opt;
    }
    if (dev < 0) ENC_TRY(hipGetDevice(&dev));
  }
  e->device = dev;
  const int rc = enc_alloc_device(e);
  if (rc) {
    enc_free_device(e);   // (a later frame tries again from nothing; nothing runs on a half-made context)
    return rc;
  }
  e->dev_ready = true;
  return 0;
}

// the allocations and uploads of enc_ensure_device, on e->device
static int enc_alloc_device(th_enc_ctx *e) {
  DeviceGuard g(e->device);
  ENC_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  ENC_TRY(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
  ENC_TRY(hipEventCreateWithFlags(&e->ev_read, hipEventDisableTiming));
  ENC_TRY(hipEventCreate(&e->ev_t0));
  ENC_TRY(hipEventCreate(&e->ev_done));
  const size_t n = (size_t)e->nfrags;
  size_t pb = 0;
  for (int p = 0; p < 3; p++) {
    e->pix_off[p] = pb;
    pb += (size_t)e->cw[p] * e->ch[p];
  }
  e->pix_bytes = pb;
  ENC_TRY(hipMalloc((void **)&e->d_pix, pb));
  ENC_TRY(hipHostMalloc((void **)&e->h_pix, pb, hipHostMallocDefault));
  ENC_TRY(hipMalloc((void **)&e->d_order, n * 4));
  ENC_TRY(hipMalloc((void **)&e->d_dequant, 64 * 3 * 64 * 2));
  ENC_TRY(hipMalloc((void **)&e->d_levels, n * 64 * 2));
  ENC_TRY(hipMalloc((void **)&e->d_dcq, n * 2));
  ENC_TRY(hipMalloc((void **)&e->d_tok, n * kEncTokWords * 4));
  ENC_TRY(hipMalloc((void **)&e->d_out, n * kEncTokWords * 4));
  ENC_TRY(hipMalloc((void **)&e->d_mask, n * 8));
  ENC_TRY(hipMalloc((void **)&e->d_cnt, (size_t)e->nchunks * 192 * 4));
  ENC_TRY(hipMalloc((void **)&e->d_base, (size_t)e->nchunks * 64 * 4));
  ENC_TRY(hipMalloc((void **)&e->d_small, 256 * 4));
  ENC_TRY(hipHostMalloc((void **)&e->h_small, 256 * 4, hipHostMallocDefault));
  std::vector<uint16_t> dq(64 * 3 * 64);
  for (int qi = 0; qi < 64; qi++)
    for (int p = 0; p < 3; p++)
      compute_qmat(e->setup.qp, 0, p, qi, &dq[(qi * 3 + p) * 64]);
  ENC_TRY(hipMemcpy(e->d_order, e->coded_order.data(), n * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(e->d_dequant, dq.data(), dq.size() * 2, hipMemcpyHostToDevice));
  if (!e->inter) return 0;   // (nothing more exists with inter frames off)
  ENC_TRY(hipMalloc((void **)&e->d_mb, (size_t)e->nmbs * 4));
  ENC_TRY(hipMalloc((void **)&e->d_dclast, (size_t)e->nchunks * 3 * 4));   // (two classes, or three with all eight modes)
  ENC_TRY(hipMalloc((void **)&e->d_cmap, n));
  ENC_TRY(hipMalloc((void **)&e->d_dcr, n * 2));
  ENC_TRY(hipMalloc((void **)&e->d_dqi, 64 * 6 * 64 * 2));
  ENC_TRY(hipHostMalloc((void **)&e->h_mb, (size_t)e->nmbs * 4, hipHostMallocDefault));
  ENC_TRY(hipHostMalloc((void **)&e->h_cmap, n, hipHostMallocDefault));
  std::vector<uint16_t> dqi(64 * 6 * 64);
  for (int qi = 0; qi < 64; qi++)
    for (int t = 0; t < 6; t++) compute_qmat(e->setup.qp, t / 3, t % 3, qi, &dqi[(qi * 6 + t) * 64]);   // intra, inter of each plane
  ENC_TRY(hipMemcpy(e->d_dqi, dqi.data(), dqi.size() * 2, hipMemcpyHostToDevice));
  return 0;
}

// the plane sizes a ycbcr buffer may have: the frame's (0) or the picture's (1); -1 neither
static int enc_buffer_kind(const th_enc_ctx *e, const th_img_plane *y) {
  for (int kind = 0; kind < 2; kind++) {
    bool ok = true;
    for (int p = 0; p < 3 && ok; p++) {
      const int w = kind ? e->cw[p] : e->nh[p] * 8, h = kind ? e->ch[p] : e->nv[p] * 8;
      ok = y[p].width == w && y[p].height == h && y[p].data != nullptr;
    }
    if (ok) return kind;
  }
  return -1;
}

// a reference of the encoder's own decoder (PREV: the previous frame; GOLD: the last key frame) as the device stage reads it
static int enc_ref_frame(th_enc_ctx *e, EncRef &R, int which = THIP_FRAME_PREV) {
  thip_state *st = thip_dec_backend(e->dec);
  const int prev = st ? thip_state_ref_idx(st, which) : -1;
  if (prev < 0) return TH_EFAULT;
  thip_plane_geom geom[3];
  if (thip_state_get_geom(st, geom, nullptr, nullptr)) return TH_EFAULT;
  const uint8_t *base = thip_state_frame_ptr(st, prev);
  for (int p = 0; p < 3; p++) {
    R.plane[p] = base + geom[p].plane_off;
    R.stride[p] = geom[p].stride;
    R.w[p] = geom[p].width;
    R.h[p] = geom[p].height;
  }
  R.hdec = e->hdec;
  R.vdec = e->vdec;
  return 0;
}

// the frame's qi list (theoraenc_hip.h, "Block-level qi"; one qi with block qi off) and, with block qi on, the selection of the
// block-qi kernels (thip_encode_bqi.h); their buffers at the first such frame (TH_ENCCTL_THIP_SET_BLOCK_QI never touches the GPU).
// An inter frame with the skip decision on, and any frame with the level choice on, runs the same selection, with a one-entry list
// where block qi is off
static int enc_bqi_prepare(th_enc_ctx *e, BqiSel &sel) {
  const int q0 = e->frame_qi;
  e->fnqis = 1;
  e->fqis[0] = q0;
  e->fqis[1] = e->fqis[2] = 0;
  if (!e->bqi && !(e->skip && !e->frame_key) && !e->rdq) return 0;
  const int coarse = std::max(q0 - e->bqi, 0), fine = std::min(q0 + e->bqi, 63);
  if (coarse != q0) e->fqis[e->fnqis++] = coarse;   // (block qi off: q0 alone)
  if (fine != q0 && fine != coarse) e->fqis[e->fnqis++] = fine;
  if (!e->d_qii) {
    ENC_TRY(hipMalloc((void **)&e->d_qii, (size_t)e->nfrags));
    ENC_TRY(hipHostMalloc((void **)&e->h_qii, (size_t)e->nfrags, hipHostMallocDefault));
    ENC_TRY(hipMalloc((void **)&e->d_bqbits, 16 * 4 * 32));
    std::vector<uint8_t> bits(16 * 4 * 32);   // [table][Huffman group - 1][token]: code length + extra bits
    for (int t = 0; t < 16; t++)
      for (int hg = 1; hg < 5; hg++)
        for (int tok = 0; tok < 32; tok++) bits[(t * 4 + hg - 1) * 32 + tok] = (uint8_t)(e->setup.len[16 * hg + t][tok] + kTokExtraBits[tok]);
    ENC_TRY(hipMemcpy(e->d_bqbits, bits.data(), bits.size(), hipMemcpyHostToDevice));
  }
  const int ft = e->frame_key ? 0 : 1;
  sel = BqiSel{e->fnqis, e->fqis[0], e->fqis[1], e->fqis[2], e->bqi_hti[ft][0], e->bqi_hti[ft][1]};
  return 0;
}

// activity masking (thip_encode_mask.h), with block qi on: the activity of the frame's source and every fragment's scale, queued in
// front of the block-qi kernel; A and the largest activity go to d_small behind the list lengths and come back with them
// (enc_queue_tail).  The buffers at the first such frame (TH_ENCCTL_THIP_SET_MASKING never touches the GPU)
static int enc_mask_queue(th_enc_ctx *e, const EncPlanes &g) {
  e->mask_queued = false;
  if (!e->mask || !e->bqi) return 0;
  const int64_t nluma = (int64_t)e->nh[0] * e->nv[0];
  if (!e->d_act) {
    for (hipEvent_t *ev : {&e->ev_a0, &e->ev_a1})
      if (!*ev) ENC_TRY(hipEventCreate(ev));
    ENC_TRY(hipMalloc((void **)&e->d_mpart, (size_t)mask_parts(nluma) * sizeof(MaskPart)));
    ENC_TRY(hipMalloc((void **)&e->d_act, (size_t)nluma * 4));
  }
  if (!e->d_iscale) ENC_TRY(hipMalloc((void **)&e->d_iscale, (size_t)e->nfrags * 2));   // (enc_roi_queue's too)
  ENC_TRY(hipEventRecord(e->ev_a0, e->stream));
  ENC_TRY(mask_launch_act(e->d_act, e->d_mpart, g, e->stream));
  ENC_TRY(mask_launch_scale(e->d_iscale, (MaskRec *)(e->d_small + kEncSmallMask), e->d_act, e->d_mpart, g, e->nfrags, e->mask, e->stream));
  ENC_TRY(hipEventRecord(e->ev_a1, e->stream));
  e->mask_queued = true;
  return 0;
}

// the last packet's thip_enc_mask_stats: those of a frame coded without masking, or (queued: after the frame's wait) the frame's own
static void enc_mask_stats(th_enc_ctx *e, bool queued) {
  memset(&e->kstats, 0, sizeof(e->kstats));
  e->kstats.ratio = e->mask;
  if (!queued) return;
  float ms = 0;
  e->kstats.measured = 1;
  const MaskRec *rec = (const MaskRec *)(e->h_small + kEncSmallMask);
  e->kstats.activity_avg = (int64_t)rec->avg;
  e->kstats.activity_max = (int64_t)rec->max;
  e->kstats.mask_ms = hipEventElapsedTime(&ms, e->ev_a0, e->ev_a1) == hipSuccess ? ms : 0.0;
}

// region of interest (thip_encode_roi.h), with block qi on and a map in force: every fragment's final scale -- on top of masking's,
// whose launches the caller has queued -- in front of the block-qi kernel; the frame's extremes go to d_small behind masking's record
// and come back with it (enc_queue_tail).  No host wait
static int enc_roi_queue(th_enc_ctx *e, const EncPlanes &g) {
  e->roi_queued = false;
  if (!e->roi_on || !e->bqi) return 0;
  if (!e->d_roipart) {
    for (hipEvent_t *ev : {&e->ev_o0, &e->ev_o1})
      if (!*ev) ENC_TRY(hipEventCreate(ev));
    ENC_TRY(hipMalloc((void **)&e->d_roipart, (size_t)roi_parts(e->nfrags) * sizeof(RoiPart)));
  }
  if (!e->d_iscale) ENC_TRY(hipMalloc((void **)&e->d_iscale, (size_t)e->nfrags * 2));   // (enc_mask_queue's too)
  ENC_TRY(hipEventRecord(e->ev_o0, e->stream));
  ENC_TRY(roi_launch_scale(e->d_iscale, e->mask_queued ? (const uint16_t *)e->d_iscale : nullptr, e->d_roipart,
                           (RoiRec *)(e->d_small + kEncSmallRoi), e->d_roimap, e->roi_w, e->roi_h, e->roi_w, e->d_roiclamp, g, e->nfrags,
                           e->stream));
  ENC_TRY(hipEventRecord(e->ev_o1, e->stream));
  e->roi_queued = true;
  return 0;
}

// the last packet's thip_enc_roi_stats: those of a frame coded without a map, or (queued: after the frame's wait) the frame's own
static void enc_roi_stats(th_enc_ctx *e, bool queued) {
  memset(&e->ostats, 0, sizeof(e->ostats));
  e->ostats.active = e->roi_on ? 1 : 0;
  e->ostats.map_width = e->roi_on ? e->roi_w : 0;
  e->ostats.map_height = e->roi_on ? e->roi_h : 0;
  if (!queued) return;
  float ms = 0;
  const RoiRec *rec = (const RoiRec *)(e->h_small + kEncSmallRoi);
  e->ostats.measured = 1;
  e->ostats.exp_min = rec->exp_min;
  e->ostats.exp_max = rec->exp_max;
  e->ostats.exp_sum = rec->exp_sum;
  e->ostats.scale_min = (int32_t)rec->scale_min;
  e->ostats.scale_max = (int32_t)rec->scale_max;
  e->ostats.clamped = (int32_t)rec->clamped;
  e->ostats.roi_ms = hipEventElapsedTime(&ms, e->ev_o0, e->ev_o1) == hipSuccess ? ms : 0.0;
}

// the scales the frame queued has in d_iscale (masking's, the map's, or both), or nullptr: the plain block-qi forms
static const uint16_t *enc_iscale(const th_enc_ctx *e) { return e->mask_queued || e->roi_queued ? e->d_iscale : nullptr; }

// what the quantising launch (fq_launch_key, fq_launch_inter of thip_encode_mask.h) selects by: the frame's list with block qi on,
// else the plain kernel at the frame's qi -- also where the skip decision or the level choice made sel a one-entry list
static BqiSel enc_fq_sel(const th_enc_ctx *e, const BqiSel &sel) { return e->bqi ? sel : BqiSel{0, e->frame_qi, 0, 0, 0, 0}; }

// TH_ENCCTL_THIP_SET_ROI_MAP, its checks made: the encoder's tight copy of the map.  A host map goes up before the call returns; a
// device map is copied, clamped and counted behind the caller's stream, which then waits for the copy alone
static int enc_roi_set(th_enc_ctx *e, const thip_enc_roi_map *a) {
  if (enc_ensure_device(e)) return TH_EFAULT;
  DeviceGuard g(e->device);
  const size_t bytes = (size_t)a->width * a->height;
  if (!e->d_roiclamp) ENC_TRY(hipMalloc((void **)&e->d_roiclamp, 4));
  if (e->roi_cap < bytes) {
    e->roi_on = false;
    if (e->d_roimap) ENC_TRY(hipFree(e->d_roimap));   // (no frame is pending: nothing reads it)
    e->d_roimap = nullptr;
    e->roi_cap = 0;
    ENC_TRY(hipMalloc((void **)&e->d_roimap, bytes));
    e->roi_cap = bytes;
  }
  if (a->device) {
    hipStream_t cs = (hipStream_t)a->stream;
    if (!e->ev_conv) ENC_TRY(hipEventCreateWithFlags(&e->ev_conv, hipEventDisableTiming));
    ENC_TRY(hipEventRecord(e->ev_in, cs));
    ENC_TRY(hipStreamWaitEvent(e->stream, e->ev_in, 0));
    ENC_TRY(roi_launch_copy(e->d_roimap, e->d_roiclamp, a->map, a->pitch, a->width, a->height, e->stream));
    ENC_TRY(hipEventRecord(e->ev_conv, e->stream));   // the caller's map has been read
    ENC_TRY(hipStreamWaitEvent(cs, e->ev_conv, 0));
  } else {
    ENC_TRY(hipMemsetAsync(e->d_roiclamp, 0, 4, e->stream));
    ENC_TRY(hipMemcpy2DAsync(e->d_roimap, (size_t)a->width, a->pitch < 0 ? a->map + (int64_t)(a->height - 1) * a->pitch : a->map,
                             (size_t)(a->pitch < 0 ? -a->pitch : a->pitch), (size_t)a->width, (size_t)a->height, hipMemcpyHostToDevice,
                             e->stream));
    ENC_TRY(hipStreamSynchronize(e->stream));   // (the caller's memory is free at return)
  }
  e->roi_w = a->width;
  e->roi_h = a->height;
  e->roi_on = true;
  e->ostats.active = 1;
  e->ostats.map_width = a->width;
  e->ostats.map_height = a->height;
  return 0;
}

// the rate-distortion mode decision in place of k_enc_me_all's (thip_encode_rd.h): the candidates, then the choice into d_mb4.  Its
// buffers and the bits table at the first such frame (TH_ENCCTL_THIP_SET_RD_MODES never touches the GPU); no host wait
static int enc_rd_queue(th_enc_ctx *e, const EncPlanes &g, const EncRef &R, const EncRef &G) {
  if (!e->d_cand) {
    for (hipEvent_t *ev : {&e->ev_r0, &e->ev_r1})
      if (!*ev) ENC_TRY(hipEventCreate(ev));
    ENC_TRY(hipMalloc((void **)&e->d_cand, (size_t)e->nmbs * 2 * sizeof(uint4)));
    ENC_TRY(hipMalloc((void **)&e->d_rdbits, 16 * 5 * 32));
    std::vector<uint8_t> bits(16 * 5 * 32);
    for (int t = 0; t < 16; t++)
      for (int hg = 0; hg < 5; hg++)
        for (int tok = 0; tok < 32; tok++) bits[(t * 5 + hg) * 32 + tok] = (uint8_t)(e->setup.len[16 * hg + t][tok] + kTokExtraBits[tok]);
    ENC_TRY(hipMemcpy(e->d_rdbits, bits.data(), bits.size(), hipMemcpyHostToDevice));
  }
  e->rd_lam = rd_lambda(e->lambda[e->frame_qi]);
  for (int c = 0; c < 4; c++) e->rd_used[c] = e->rd_hti[c];
  ENC_TRY(hipEventRecord(e->ev_r0, e->stream));
  ENC_TRY(rd_launch(RdBufs{e->d_cand, e->d_mb4, nullptr}, true, true, g, R, G, e->nmbx, e->nmbs, e->lambda[e->frame_qi], e->rd_lam,
                    e->d_dqi + (size_t)e->frame_qi * 384, e->d_rdbits, make_int4(e->rd_hti[0], e->rd_hti[1], e->rd_hti[2], e->rd_hti[3]),
                    e->stream));
  ENC_TRY(hipEventRecord(e->ev_r1, e->stream));
  e->rd_queued = true;
  return 0;
}

// the last packet's thip_enc_rd_stats: those of a frame not decided this way, or (queued: after the frame's wait) the frame's own
static void enc_rd_stats(th_enc_ctx *e, bool queued) {
  memset(&e->dstats, 0, sizeof(e->dstats));
  e->dstats.on = e->rd ? 1 : 0;
  if (!queued) return;
  float ms = 0;
  e->dstats.measured = 1;
  for (int c = 0; c < 4; c++) e->dstats.huff[c] = e->rd_used[c];
  e->dstats.lambda = e->rd_lam;
  e->dstats.rd_ms = hipEventElapsedTime(&ms, e->ev_r0, e->ev_r1) == hipSuccess ? ms : 0.0;
}

// the skip decision (thip_encode_skip.h): its two launches in place of the frame's quantising kernel, between HIP events.  The flags
// and the events at the first such frame (TH_ENCCTL_THIP_SET_RD_SKIP never touches the GPU); no host wait
extern "C++" template <class Word>
static int enc_skip_queue(th_enc_ctx *e, const EncPlanes &g, const BqiSel &sel, const Word *d_mb, const EncRef &R, const EncRef &G) {
  if (!e->d_skf) {
    for (hipEvent_t *ev : {&e->ev_s0, &e->ev_s1})
      if (!*ev) ENC_TRY(hipEventCreate(ev));
    ENC_TRY(hipMalloc((void **)&e->d_skf, (size_t)e->nfrags));
    ENC_TRY(hipHostMalloc((void **)&e->h_skf, (size_t)e->nfrags, hipHostMallocDefault));
  }
  e->skip_lam = rd_lambda(e->lambda[e->frame_qi]);
  ENC_TRY(hipEventRecord(e->ev_s0, e->stream));
  ENC_TRY(skip_launch(InterBufs{e->d_levels, e->d_dcq, e->d_cmap, e->d_dclast, e->d_small + 192}, e->d_qii,
                      SkipOut{e->d_skf, nullptr, nullptr, nullptr}, e->d_order, g, R, G, d_mb, e->nmbx, e->d_dqi, e->d_bqbits, sel,
                      enc_iscale(e), -1, e->nfrags, e->stream));
  ENC_TRY(hipEventRecord(e->ev_s1, e->stream));
  e->skip_queued = true;
  return 0;
}

// the last packet's thip_enc_skip_stats: those of a frame not decided this way, or (queued: after the frame's wait) the frame's own
// from the flags and the coded map
static void enc_skip_stats(th_enc_ctx *e, bool queued) {
  memset(&e->sstats, 0, sizeof(e->sstats));
  e->sstats.on = e->skip ? 1 : 0;
  if (!queued) return;
  float ms = 0;
  e->sstats.measured = 1;
  for (int p = 0; p < 3; p++)
    for (int f = e->fro[p]; f < e->fro[p] + e->nh[p] * e->nv[p]; f++) e->sstats.skipped[p] += e->h_skf[f] != 0;
  for (const MacroBlock &m : e->mbs) {
    bool coded = false, flagged = false;
    for (int k = 0; k < 4; k++) {
      coded |= e->h_cmap[m.luma[k]] != 0;
      flagged |= e->h_skf[m.luma[k]] != 0;
    }
    e->sstats.demoted += !coded && flagged;
  }
  e->sstats.lambda = e->skip_lam;
  e->sstats.skip_ms = hipEventElapsedTime(&ms, e->ev_s0, e->ev_s1) == hipSuccess ? ms : 0.0;
}

// the level choice (thip_encode_rdq.h): its launch behind the frame's quantising (or skip) launches and in front of the DC and token
// kernels, between HIP events; classes 0 for a key frame.  The kernel reads the source once more: the caller records "the planes have
// been read" behind it.  The sums and the events at the first such frame (TH_ENCCTL_THIP_SET_RD_QUANT never touches the GPU); no
// host wait
extern "C++" template <class Word>
static int enc_rdq_queue(th_enc_ctx *e, int classes, const EncPlanes &g, const BqiSel &sel, const Word *d_mb, const EncRef &R, const EncRef &G) {
  if (!e->rdq) return 0;
  if (!e->d_rdqsums) {
    for (hipEvent_t *ev : {&e->ev_z0, &e->ev_z1})
      if (!*ev) ENC_TRY(hipEventCreate(ev));
    ENC_TRY(hipMalloc((void **)&e->d_rdqsums, kRdqSums * sizeof(unsigned long long)));
    ENC_TRY(hipHostMalloc((void **)&e->h_rdqsums, kRdqSums * sizeof(unsigned long long), hipHostMallocDefault));
  }
  uint16_t step[64];
  compute_qmat(e->setup.qp, classes ? 1 : 0, 0, e->frame_qi, step);
  e->rdq_lam = rd_lambda(step[1]);
  // the quantising kernel wrote qii with block qi on, and the skip launches always do
  const uint8_t *qii = e->bqi || e->skip_queued ? e->d_qii : nullptr;
  ENC_TRY(hipEventRecord(e->ev_z0, e->stream));
  ENC_TRY(hipMemsetAsync(e->d_rdqsums, 0, kRdqSums * sizeof(unsigned long long), e->stream));
  ENC_TRY(rdq_launch(classes, e->d_levels, qii, e->d_cmap, RdqOut{nullptr, nullptr, nullptr, e->d_rdqsums}, e->d_order, g, R, G, d_mb,
                     e->nmbx, classes ? e->d_dqi : e->d_dequant, classes ? 6 : 3, e->d_bqbits, sel,
                     enc_iscale(e), -1, e->rdq, e->nfrags, e->stream));
  ENC_TRY(hipEventRecord(e->ev_z1, e->stream));
  e->rdq_queued = true;
  return 0;
}

// the last packet's thip_enc_rd_quant_stats: those of a frame not treated, or (queued: after the frame's wait) the frame's own sums
static void enc_rdq_stats(th_enc_ctx *e, bool queued) {
  memset(&e->zstats, 0, sizeof(e->zstats));
  e->zstats.weight = e->rdq;
  if (!queued) return;
  float ms = 0;
  const unsigned long long *s = e->h_rdqsums;
  e->zstats.measured = 1;
  for (int p = 0; p < 3; p++) {
    e->zstats.zeroed[p] = (int32_t)s[kRdqZeroed + p];
    e->zstats.lowered[p] = (int32_t)s[kRdqLowered + p];
  }
  e->zstats.emptied = (int32_t)s[kRdqEmptied];
  e->zstats.rate_before = (int64_t)s[kRdqRateBefore];
  e->zstats.rate_after = (int64_t)s[kRdqRateAfter];
  e->zstats.dist_before = (int64_t)s[kRdqDistBefore];
  e->zstats.dist_after = (int64_t)s[kRdqDistAfter];
  e->zstats.lambda = e->rdq_lam;
  e->zstats.rdq_ms = hipEventElapsedTime(&ms, e->ev_z0, e->ev_z1) == hipSuccess ? ms : 0.0;
}

// ---- the device packetiser (thip_encode_pack.h) ----------------------------------------------------------------------------------
// its buffers and tables, at the first frame that needs them.  The packet buffer holds 128 bytes a block -- 16 bits a coefficient,
// twice the raw picture; the natural image of tools/encode_time.py takes 9.5 bytes a block at quality 48 -- where the worst case, 65
// tokens of 43 bits a block, would be 350.  A frame beyond it is packed by the host.
static int enc_pack_alloc(th_enc_ctx *e) {
  if (e->d_pk) return 0;
  const size_t n = (size_t)e->nfrags;
  e->pack_groups = (int)std::min(std::max(n / 64, (size_t)1), (size_t)kPackMaxGroups);
  const size_t cap = n * 128 + 64;
  for (hipEvent_t *ev : {&e->ev_k0, &e->ev_k1, &e->ev_q0, &e->ev_q1})
    if (!*ev) ENC_TRY(hipEventCreate(ev));
  ENC_TRY(hipMalloc((void **)&e->d_pglast, (size_t)e->pack_groups * 4));
  ENC_TRY(hipMalloc((void **)&e->d_pcodes, 80 * 32 * 4));
  ENC_TRY(hipMalloc((void **)&e->d_pcl, 80 * 32 * 4));
  ENC_TRY(hipMalloc((void **)&e->d_pgsum, (size_t)e->pack_groups * sizeof(PackSum)));
  ENC_TRY(hipMalloc((void **)&e->d_pgbase, (size_t)e->pack_groups * sizeof(PackSum)));
  // the record and, behind it, the histogram: one copy brings both back (thip_enc_token_hist is the histogram's)
  ENC_TRY(hipMalloc((void **)&e->d_prec, kEncPackRecBytes));
  e->d_phist = (uint32_t *)(e->d_prec + 1);
  ENC_TRY(hipHostMalloc((void **)&e->h_prec, kEncPackRecBytes, hipHostMallocDefault));
  std::vector<uint32_t> cl(80 * 32);
  pack_cl_table(cl.data(), e->setup.len);
  ENC_TRY(hipMemcpy(e->d_pcodes, e->setup.code, 80 * 32 * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(e->d_pcl, cl.data(), cl.size() * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMalloc((void **)&e->d_pk, cap));
  e->pack_cap = cap;
  return 0;
}

// the context's packetiser buffers as the launches of thip_encode_pack.h take them.  The merged words go where the tokens were
// before the scatter (d_tok is dead by then).
static PackBufs enc_pack_bufs(const th_enc_ctx *e) {
  return PackBufs{e->d_pglast, e->d_phist, e->d_pcodes, e->d_pcl, (uint32_t *)e->d_tok, e->d_pgsum, e->d_pgbase, e->d_prec};
}

// everything that does not need the header's length, queued behind k_enc_intra_scatter with no host wait: the merge, the tables,
// the scan, and the record's copy
static int enc_pack_queue(th_enc_ctx *e) {
  e->frame_dpack = false;
  if (!e->dpack || (uint64_t)e->nfrags * kEncTokWords >= (1ull << 31)) return 0;   // (token indices are 32-bit with room for i + 1)
  if (enc_pack_alloc(e)) return TH_EFAULT;
  ENC_TRY(hipEventRecord(e->ev_k0, e->stream));
  ENC_TRY(pack_launch_sums(enc_pack_bufs(e), (const uint32_t *)e->d_out, (const uint32_t *)e->d_small, e->pack_groups, e->stream));
  ENC_TRY(hipMemcpyAsync(e->h_prec, e->d_prec, kEncPackRecBytes, hipMemcpyDeviceToHost, e->stream));
  ENC_TRY(hipEventRecord(e->ev_k1, e->stream));
  e->frame_dpack = true;
  return 0;
}

// the frame queued (or dropped) is pending for th_encode_packetout, with the duplicates asked for it
static void enc_frame_queued(th_enc_ctx *e) {
  e->frame_pending = true;
  e->dups_left = e->dup_next;
  e->dup_next = 0;
}

// the context's token buffers as the launches of thip_encode.h and thip_encode_inter.h take them: the overflow count lies behind
// the list lengths in d_small
static TokBufs enc_tok_bufs(const th_enc_ctx *e) { return TokBufs{e->d_tok, e->d_mask, e->d_cnt, e->d_small + 192}; }

// everything behind the token kernel, for both frame types: the scan, the scatter, the read-backs, the device packetiser
static int enc_queue_tail(th_enc_ctx *e) {
  const int64_t n = e->nfrags;
  ENC_TRY(tok_launch_scan(e->d_base, e->d_small, e->d_cnt, n, e->stream));
  ENC_TRY(tok_launch_scatter(e->d_out, e->d_tok, e->d_mask, e->d_base, e->d_small, n, e->stream));
  // (a masked frame: its record too; a frame with a map: both places)
  const size_t nsmall = e->roi_queued ? kEncSmallRoi + sizeof(RoiRec) / 4 : e->mask_queued ? kEncSmallMask + sizeof(MaskRec) / 4 : 193;
  ENC_TRY(hipMemcpyAsync(e->h_small, e->d_small, nsmall * 4, hipMemcpyDeviceToHost, e->stream));
  if (!e->frame_key) {
    if (e->modes) ENC_TRY(hipMemcpyAsync(e->h_mb4, e->d_mb4, (size_t)e->nmbs * sizeof(uint4), hipMemcpyDeviceToHost, e->stream));
    else ENC_TRY(hipMemcpyAsync(e->h_mb, e->d_mb, (size_t)e->nmbs * 4, hipMemcpyDeviceToHost, e->stream));
    ENC_TRY(hipMemcpyAsync(e->h_cmap, e->d_cmap, (size_t)n, hipMemcpyDeviceToHost, e->stream));
  }
  if (e->bqi) ENC_TRY(hipMemcpyAsync(e->h_qii, e->d_qii, (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (e->skip_queued) ENC_TRY(hipMemcpyAsync(e->h_skf, e->d_skf, (size_t)n, hipMemcpyDeviceToHost, e->stream));
  if (e->rdq_queued)
    ENC_TRY(hipMemcpyAsync(e->h_rdqsums, e->d_rdqsums, kRdqSums * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  ENC_TRY(hipEventRecord(e->ev_done, e->stream));
  if (enc_pack_queue(e)) return TH_EFAULT;
  enc_frame_queued(e);
  return 0;
}

// the buffers of all eight modes (k_enc_me_all's words), at the first inter frame with them: TH_ENCCTL_THIP_SET_INTER_MODES never
// touches the GPU
static int enc_modes_alloc(th_enc_ctx *e) {
  if (e->d_mb4) return 0;
  ENC_TRY(hipMalloc((void **)&e->d_mb4, (size_t)e->nmbs * sizeof(uint4)));
  ENC_TRY(hipHostMalloc((void **)&e->h_mb4, (size_t)e->nmbs * sizeof(uint4), hipHostMallocDefault));
  return 0;
}

// The launches of an inter frame, written once for its two sets of kernels: the search, the transform-and-quantise and the DC
// launch of one macro-block word (d_mb) are the launch functions beside the kernels (thip_encode_inter.h, thip_encode_modes.h),
// which thip_enc_inter_stage calls too; the quantising kernel of that word is fq_launch_inter's choice (thip_encode_mask.h), which
// thip_enc_fq_stage calls too; gold: GOLD for the kernels that read it (three reference classes then), else nothing (two).
// stats: k_rate_me's words of this frame where the measurement of thip_encode_cut.h left them and d_mb follows from them (five
// modes) -- k_enc_mb_modes then stands in for the search --, else nullptr
extern "C++" template <class Word, class... Gold>
static int enc_launch_inter(th_enc_ctx *e, const EncPlanes &g, const BqiSel &sel, Word *d_mb, const uint4 *stats, const EncRef &R,
                            const Gold &...gold) {
  constexpr int classes = sizeof...(Gold) ? 3 : 2;
  const int64_t n = e->nfrags;
  const int lambda = e->lambda[e->frame_qi];
  ENC_TRY(hipEventRecord(e->ev_t0, e->stream));
  ENC_TRY(hipMemsetAsync(e->d_dclast, 0, (size_t)e->nchunks * classes * 4, e->stream));
  if (enc_mask_queue(e, g) || enc_roi_queue(e, g)) return TH_EFAULT;
  if constexpr (sizeof(Word) == sizeof(uint32_t)) {
    if (stats) ENC_TRY(cut_launch_mb_modes(d_mb, stats, e->nmbs, lambda, e->stream));
    else ENC_TRY(inter_launch_search(d_mb, g, R, e->nmbx, e->nmbs, lambda, e->stream));
  } else if (e->rd) {
    if (enc_rd_queue(e, g, R, gold...)) return TH_EFAULT;
  } else {
    ENC_TRY(inter_launch_search(d_mb, g, R, gold..., e->nmbx, e->nmbs, lambda, e->stream));
  }
  const EncRef *G[] = {&R, &gold...};   // (GOLD where the word has it, else PREV, which is not read)
  if (e->skip) {
    if (enc_skip_queue(e, g, sel, (const Word *)d_mb, R, *G[sizeof...(Gold)])) return TH_EFAULT;
  } else {
    ENC_TRY(fq_launch_inter(InterBufs{e->d_levels, e->d_dcq, e->d_cmap, e->d_dclast, e->d_small + 192}, e->d_qii, e->d_order, g, R,
                            *G[sizeof...(Gold)], (const Word *)d_mb, e->nmbx, e->d_dqi, e->d_bqbits, enc_fq_sel(e, sel), enc_iscale(e), n,
                            e->stream));
  }
  if (enc_rdq_queue(e, classes, g, sel, (const Word *)d_mb, R, *G[sizeof...(Gold)])) return TH_EFAULT;
  ENC_TRY(hipEventRecord(e->ev_read, e->stream));   // the planes have been read (the level choice reads them too)
  if constexpr (classes == 3) ENC_TRY(inter_launch_dc3(e->d_dcr, e->d_dcq, e->d_cmap, e->d_dclast, g, n, e->stream));
  else ENC_TRY(inter_launch_dc(e->d_dcr, e->d_dcq, e->d_cmap, e->d_dclast, g, n, e->stream));
  ENC_TRY(tok_launch_inter(enc_tok_bufs(e), e->d_levels, e->d_dcr, e->d_cmap, e->d_order, g, n, e->stream));
  return enc_queue_tail(e);
}

// an inter frame against the reconstruction of the previous frame (thip_encode_inter.h), with all eight modes against the last
// key frame's too (thip_encode_modes.h)
static int enc_queue_inter(th_enc_ctx *e, const EncPlanes &g, const BqiSel &sel, const uint4 *stats) {
  EncRef R, G;
  if (enc_ref_frame(e, R)) return TH_EFAULT;
  if (!e->modes) return enc_launch_inter(e, g, sel, e->d_mb, stats, R);
  if (enc_ref_frame(e, G, THIP_FRAME_GOLD) || enc_modes_alloc(e)) return TH_EFAULT;
  return enc_launch_inter(e, g, sel, e->d_mb4, nullptr, R, G);
}

// ---- bitrate mode -----------------------------------------------------------------------------------------------------------
// the probe's buffers, at the first frame in bitrate mode
static int enc_rate_alloc(th_enc_ctx *e) {
  if (e->rate_dev) return 0;
  const int64_t n = e->nfrags;
  ENC_TRY(hipEventCreate(&e->ev_p0));
  ENC_TRY(hipEventCreate(&e->ev_p1));
  e->rate_nwg = rate_groups(n);
  ENC_TRY(hipMalloc((void **)&e->d_coef, (size_t)(e->inter ? 3 : 1) * n * 64 * 2));
  ENC_TRY(hipMalloc((void **)&e->d_qdc, (size_t)n * 64 * 2));
  ENC_TRY(hipMalloc((void **)&e->d_rcoded, (size_t)n * 8));
  ENC_TRY(hipMalloc((void **)&e->d_rcls, (size_t)n * 8));
  if (!e->d_rmbs) ENC_TRY(hipMalloc((void **)&e->d_rmbs, (size_t)std::max(e->nmbs, 1) * sizeof(uint4)));   // (enc_cut_alloc's, else)
  ENC_TRY(hipMalloc((void **)&e->d_rtab, 6 * 64 * 64 * sizeof(uint2) + 6 * 64 * sizeof(uint16_t)));   // the table, then its floor
  ENC_TRY(hipMalloc((void **)&e->d_rlam, 64 * sizeof(int)));
  ENC_TRY(hipMalloc((void **)&e->d_rlens, 80 * 32));
  ENC_TRY(hipMalloc((void **)&e->d_rpart, (size_t)e->rate_nwg * 64 * kRatePartial * 4));
  ENC_TRY(hipMalloc((void **)&e->d_rest, 64 * 8));
  ENC_TRY(hipHostMalloc((void **)&e->h_rest, 64 * 8, hipHostMallocDefault));
  std::vector<uint16_t> steps(6 * 64 * 64), floor(6 * 64);
  quant_all_steps(e->setup.qp, steps.data());
  if (!rate_steps_ok(steps.data(), true)) return TH_EFAULT;   // (qmin and the cap of spec 6.4.3 keep every step in 8..4096)
  std::vector<uint2> tab(6 * 64 * 64);
  rate_form_table(tab.data(), steps.data());
  rate_form_floor(floor.data(), steps.data());
  ENC_TRY(hipMemcpy(e->d_rtab, tab.data(), tab.size() * sizeof(uint2), hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(e->d_rtab + tab.size(), floor.data(), floor.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(e->d_rlam, e->lambda, sizeof(e->lambda), hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(e->d_rlens, e->setup.len, 80 * 32, hipMemcpyHostToDevice));
  e->rate_dev = true;
  return 0;
}

// the probe's 512 bytes are on the host (ev_p1 has passed): the controller's E, and the probe's device time
static void enc_rate_read(th_enc_ctx *e) {
  float ms = 0;
  e->ratectl.stats.probe_ms = hipEventElapsedTime(&ms, e->ev_p0, e->ev_p1) == hipSuccess ? ms : 0.0;
  memcpy(e->ratectl.E, e->h_rest, sizeof(e->ratectl.E));
}

// E[0..63] of the frame about to be coded (thip_rate.h) into the controller's E: queued on the encoder's stream behind its input,
// waited for.  searched: d_rmbs holds k_rate_me's words of this frame already (enc_cut_measure).  wait = false (pass 1 of two-pass
// in quality mode): nothing is waited for; the 512 bytes are in h_rest once ev_p1 has passed (enc_2pass_collect)
static int enc_rate_probe(th_enc_ctx *e, const EncPlanes &g, bool key, bool searched, bool wait = true) {
  const int64_t n = e->nfrags;
  RateArgs a;
  a.coef = e->d_coef;
  a.tab = e->d_rtab;
  a.mbs = e->d_rmbs;
  a.lam = e->d_rlam;
  a.floor = (const uint16_t *)(e->d_rtab + 6 * 64 * 64);
  a.nmbx = e->nmbx;
  a.hdec = e->hdec;
  a.vdec = e->vdec;
  ENC_TRY(hipEventRecord(e->ev_p0, e->stream));
  if (key) {
    ENC_TRY(rate_launch_coef(e->d_coef, g, n, e->stream));
  } else {
    EncRef R;
    if (enc_ref_frame(e, R)) return TH_EFAULT;
    if (!searched) {
      ENC_TRY(rate_launch_me(e->d_rmbs, g, R, e->nmbx, e->nmbs, e->stream));
    }
    ENC_TRY(rate_launch_coef(e->d_coef, g, R, (const uint4 *)e->d_rmbs, e->nmbx, n, e->stream));
  }
  ENC_TRY(rate_launch_dc(!key, e->d_qdc, e->d_rcoded, e->d_rcls, a, g, n, e->stream));
  ENC_TRY(rate_launch_tok(!key, e->d_rpart, e->rate_nwg, e->d_qdc, e->d_rcoded, e->d_rcls, a, g, n, e->stream));
  // header bits: 0, frame type, qi, 0 (+ 3 reserved bits in a key frame) and the four table indices; an inter frame adds nfrags / 8
  const int fixed = key ? 12 + 16 : 9 + 16 + (int)(n / 8);
  ENC_TRY(rate_launch_bits(e->d_rest, (const uint32_t *)e->d_rpart, e->rate_nwg, (const uint8_t *)e->d_rlens, fixed, e->stream));
  ENC_TRY(hipMemcpyAsync(e->h_rest, e->d_rest, 64 * 8, hipMemcpyDeviceToHost, e->stream));
  ENC_TRY(hipEventRecord(e->ev_p1, e->stream));
  if (!wait) return 0;
  ENC_TRY(hipEventSynchronize(e->ev_p1));
  enc_rate_read(e);
  return 0;
}

// pass 1, quality mode: the probe queued with the frame has its 512 bytes on the host
static int enc_2pass_collect(th_enc_ctx *e) {
  if (!e->probe_queued) return 0;
  e->probe_queued = false;
  const double t0 = thip_now();
  ENC_TRY(hipEventSynchronize(e->ev_p1));
  e->twopass.stats.wait_ms = (thip_now() - t0) * 1e3;
  enc_rate_read(e);
  return 0;
}

// what the controllers read of the stream (thip_ratectl.h)
static EncStream enc_stream(const th_enc_ctx *e) {
  const th_info &i = e->info;
  return {i.frame_width, i.frame_height, i.pic_x, i.pic_y, i.pic_width, i.pic_height, (uint32_t)i.pixel_fmt, i.fps_numerator,
          i.fps_denominator, i.keyframe_granule_shift, e->inter, e->kf_interval, e->cur, e->key, e->dup_next, e->frame_qi,
          e->frame_pending, e->dups_left};
}

// ---- automatic key frames (thip_encode_cut.h) ---------------------------------------------------------------------------------------
// the measurement's buffers, at the first frame measured: TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES never touches the GPU
static int enc_cut_alloc(th_enc_ctx *e) {
  if (e->d_cut) return 0;
  for (hipEvent_t *ev : {&e->ev_c0, &e->ev_c1})
    if (!*ev) ENC_TRY(hipEventCreate(ev));
  if (!e->d_rmbs) ENC_TRY(hipMalloc((void **)&e->d_rmbs, (size_t)std::max(e->nmbs, 1) * sizeof(uint4)));   // (enc_rate_alloc's, else)
  if (!e->h_cut) ENC_TRY(hipHostMalloc((void **)&e->h_cut, sizeof(CutSums), hipHostMallocDefault));
  ENC_TRY(hipMalloc((void **)&e->d_cut, sizeof(CutSums)));
  return 0;
}

// P, I and N of the frame about to be coded against PREV into e->cnext, and the decision: queued on the encoder's stream behind its
// input, waited for.  k_rate_me's words stay in d_rmbs for the frame's own launches and for the probe.
static int enc_cut_measure(th_enc_ctx *e, const EncPlanes &g) {
  if (enc_cut_alloc(e)) return TH_EFAULT;
  EncRef R;
  if (enc_ref_frame(e, R)) return TH_EFAULT;
  ENC_TRY(hipEventRecord(e->ev_c0, e->stream));
  ENC_TRY(hipMemsetAsync(e->d_cut, 0, sizeof(CutSums), e->stream));
  ENC_TRY(rate_launch_me(e->d_rmbs, g, R, e->nmbx, e->nmbs, e->stream));
  hipLaunchKernelGGL(k_enc_cut_sums, dim3((unsigned)((e->nmbs + 255) / 256)), dim3(256), 0, e->stream, e->d_cut, (const uint4 *)e->d_rmbs,
                     e->nmbs);
  ENC_TRY(hipGetLastError());
  ENC_TRY(hipMemcpyAsync(e->h_cut, e->d_cut, sizeof(CutSums), hipMemcpyDeviceToHost, e->stream));
  ENC_TRY(hipEventRecord(e->ev_c1, e->stream));
  ENC_TRY(hipEventSynchronize(e->ev_c1));
  float ms = 0;
  thip_enc_cut_stats &c = e->cnext;
  c.measured = 1;
  c.pred = (int64_t)e->h_cut->pred;
  c.intra = (int64_t)e->h_cut->intra;
  c.intra_mbs = (int32_t)e->h_cut->nintra;
  c.cut = 256 * c.pred >= (int64_t)e->auto_kf * c.intra && c.pred >= (int64_t)4 * 256 * e->nmbs;
  c.measure_ms = hipEventElapsedTime(&ms, e->ev_c0, e->ev_c1) == hipSuccess ? ms : 0.0;
  return 0;
}

// the four launches of a frame, reading the picture through `src` / `stride` (top-left pixel of the picture of each plane)
static int enc_queue_frame(th_enc_ctx *e, const uint8_t *const src[3], const int64_t stride[3]) {
  const th_info &i = e->info;
  const EncPlanes g = enc_planes(*e, PicRect{(int)i.pic_x, (int)i.pic_y, (int)i.pic_width, (int)i.pic_height}, src, stride);
  const int64_t n = e->nfrags;
  e->mask_queued = false;   // (enc_mask_queue says otherwise; a dropped frame never gets there)
  e->roi_queued = false;    // (enc_roi_queue likewise)
  e->rd_queued = false;     // (enc_rd_queue likewise)
  e->skip_queued = false;   // (enc_skip_queue likewise)
  e->rdq_queued = false;    // (enc_rdq_queue likewise)
  if (!e->rate) e->frame_qi = e->qi;   // (bitrate mode: the controller's choice, below)
  // a key frame: the first, every kf_interval-th (duplicates counted), and one whose duplicates would reach 1 << shift
  const int64_t f = e->cur + 1, off = f - e->key, full = (int64_t)1 << e->info.keyframe_granule_shift;
  e->frame_key = !e->inter || e->key < 0 || off >= e->kf_interval || off + e->dup_next >= full;
  // automatic key frames: an inter frame by that rule is measured first, and a cut makes it a key frame in every respect
  memset(&e->cnext, 0, sizeof(e->cnext));
  e->cnext.ratio = e->auto_kf;
  bool searched = false;   // d_rmbs holds this frame's search
  if (e->twopass.pass == 2) {
    // the second pass: the type is the record's; neither the interval nor a measurement is consulted
    e->frame_key = e->twopass.type(enc_stream(e), f);
  } else if (e->auto_kf && !e->frame_key) {
    const int mrc = enc_cut_measure(e, g);
    if (mrc) return mrc;
    e->frame_key = e->cnext.cut != 0;
    searched = !e->frame_key;
  }
  e->probe_queued = false;
  if (e->twopass.pass == 1 && !e->rate) {
    // the first pass in quality mode: the probe's launches in front of the frame's, its 512 bytes read in th_encode_packetout
    if (enc_rate_alloc(e)) return TH_EFAULT;
    const int prc = enc_rate_probe(e, g, e->frame_key, searched, false);
    if (prc) return prc;
    e->probe_queued = true;
  }
  if (e->rate) {
    // bitrate mode: the probe, then the controller's qi -- or a dropped frame, a zero-byte packet with nothing more queued
    if (enc_rate_alloc(e)) return TH_EFAULT;
    const int prc = enc_rate_probe(e, g, e->frame_key, searched);
    if (prc) return prc;
    ENC_TRY(hipEventRecord(e->ev_read, e->stream));   // the planes have been read (the launches below record it again)
    const double t0 = thip_now();
    const EncStream s = enc_stream(e);
    const int qi = e->twopass.pass == 2 ? e->twopass.choose(s, e->ratectl, e->frame_key)
                                        : e->ratectl.choose(s, e->frame_key, f, e->frame_key ? f : e->key);
    e->ratectl.stats.control_ms = (thip_now() - t0) * 1e3;
    if (qi < 0) {
      e->frame_key = false;
      e->cnext.cut = 0;   // (a dropped frame is not a key frame, whatever was measured)
      e->frame_dpack = false;
      e->rate_dropped = true;
      enc_frame_queued(e);
      return 0;
    }
    e->frame_qi = qi;
  }
  BqiSel sel{};
  if (enc_bqi_prepare(e, sel)) return TH_EFAULT;
  if (!e->frame_key) return enc_queue_inter(e, g, sel, searched ? (const uint4 *)e->d_rmbs : nullptr);
  ENC_TRY(hipEventRecord(e->ev_t0, e->stream));
  if (enc_mask_queue(e, g) || enc_roi_queue(e, g)) return TH_EFAULT;
  ENC_TRY(fq_launch_key(e->d_levels, e->d_dcq, e->d_qii, e->d_small + 192, e->d_order, g, e->d_dequant, e->d_bqbits, enc_fq_sel(e, sel),
                        enc_iscale(e), n, e->stream));
  if (enc_rdq_queue(e, 0, g, sel, (const uint32_t *)nullptr, EncRef{}, EncRef{})) return TH_EFAULT;
  ENC_TRY(hipEventRecord(e->ev_read, e->stream));   // the planes have been read (the level choice reads them too)
  ENC_TRY(tok_launch_intra(enc_tok_bufs(e), e->d_levels, e->d_dcq, e->d_order, g, n, e->stream));
  return enc_queue_tail(e);
}

int th_encode_ycbcr_in(th_enc_ctx *e, th_ycbcr_buffer ycbcr) {
  if (!e || !ycbcr) return TH_EFAULT;
  if (e->done || e->frame_pending || e->dups_left || e->twopass.gate(enc_stream(e))) return TH_EINVAL;
  const int kind = enc_buffer_kind(e, ycbcr);
  if (kind < 0) return TH_EINVAL;
  if (enc_ensure_device(e)) return TH_EFAULT;
  DeviceGuard g(e->device);
  // the previous frame's upload is complete (its packet is out), so the staging buffer is free
  const uint8_t *src[3];
  int64_t stride[3];
  for (int p = 0; p < 3; p++) {
    const uint8_t *in = ycbcr[p].data;
    if (kind == 0) in += (int64_t)e->cy0[p] * ycbcr[p].stride + e->cx0[p];
    uint8_t *dst = e->h_pix + e->pix_off[p];
    for (int y = 0; y < e->ch[p]; y++) memcpy(dst + (size_t)y * e->cw[p], in + (int64_t)y * ycbcr[p].stride, (size_t)e->cw[p]);
    src[p] = e->d_pix + e->pix_off[p];
    stride[p] = e->cw[p];
  }
  ENC_TRY(hipMemcpyAsync(e->d_pix, e->h_pix, e->pix_bytes, hipMemcpyHostToDevice, e->stream));
  return enc_queue_frame(e, src, stride);
}

static int enc_ycbcr_in_device(th_enc_ctx *e, const thip_enc_device_in *a) {
  if (e->done || e->frame_pending || e->dups_left || e->twopass.gate(enc_stream(e))) return TH_EINVAL;
  const int kind = enc_buffer_kind(e, a->planes);
  if (kind < 0) return TH_EINVAL;
  if (enc_ensure_device(e)) return TH_EFAULT;
  DeviceGuard g(e->device);
  const uint8_t *src[3];
  int64_t stride[3];
  for (int p = 0; p < 3; p++) {
    src[p] = a->planes[p].data + (kind == 0 ? (int64_t)e->cy0[p] * a->planes[p].stride + e->cx0[p] : 0);
    stride[p] = a->planes[p].stride;
  }
  hipStream_t cs = (hipStream_t)a->stream;
  ENC_TRY(hipEventRecord(e->ev_in, cs));
  ENC_TRY(hipStreamWaitEvent(e->stream, e->ev_in, 0));
  if (e->qflags) {   // the source has to outlive the call for the packet's compare: the frame is coded from a copy in d_pix
    if (!e->ev_conv) ENC_TRY(hipEventCreateWithFlags(&e->ev_conv, hipEventDisableTiming));
    for (int p = 0; p < 3; p++) {
      ENC_TRY(hipMemcpy2DAsync(e->d_pix + e->pix_off[p], (size_t)e->cw[p], src[p], (size_t)stride[p], (size_t)e->cw[p], (size_t)e->ch[p],
                               hipMemcpyDeviceToDevice, e->stream));
      src[p] = e->d_pix + e->pix_off[p];
      stride[p] = e->cw[p];
    }
    ENC_TRY(hipEventRecord(e->ev_conv, e->stream));   // the caller's planes have been read
    ENC_TRY(hipStreamWaitEvent(cs, e->ev_conv, 0));
    return enc_queue_frame(e, src, stride);
  }
  const int rc = enc_queue_frame(e, src, stride);
  if (rc) return rc;
  ENC_TRY(hipStreamWaitEvent(cs, e->ev_read, 0));
  return 0;
}

// TH_ENCCTL_THIP_RGB_IN: the picture through thip_picture_in into d_pix (picture-sized planes, stride cw[p]), then the frame as ever
static int enc_rgb_in(th_enc_ctx *e, const thip_enc_rgb_in *a) {
  if (e->done || e->frame_pending || e->dups_left || e->twopass.gate(enc_stream(e))) return TH_EINVAL;
  if (a->format != THIP_PIC_RGB24 && a->format != THIP_PIC_RGBA32 && a->format != THIP_PIC_RGB_PLANAR) return TH_EINVAL;
  if (a->device != 0 && a->device != 1) return TH_EINVAL;
  if (a->width != (int32_t)e->info.pic_width || a->height != (int32_t)e->info.pic_height) return TH_EINVAL;
  const int ns = a->format == THIP_PIC_RGB_PLANAR ? 3 : 1;
  const int64_t row = (int64_t)a->width * (a->format == THIP_PIC_RGB24 ? 3 : a->format == THIP_PIC_RGBA32 ? 4 : 1);
  for (int p = 0; p < ns; p++)
    if (!a->src[p]) return TH_EFAULT;
  for (int p = 0; p < ns; p++)
    if (a->pitch[p] < row) return TH_EINVAL;
  if (enc_ensure_device(e)) return TH_EFAULT;
  DeviceGuard g(e->device);
  thip_picture_in_req q;
  memset(&q, 0, sizeof(q));
  q.format = a->format;
  q.pixel_fmt = (int32_t)e->info.pixel_fmt;
  q.pic_x = (int32_t)e->info.pic_x;
  q.pic_y = (int32_t)e->info.pic_y;
  q.width = a->width;
  q.height = a->height;
  const uint8_t *src[3];
  int64_t stride[3];
  for (int p = 0; p < 3; p++) {
    q.dst[p] = e->d_pix + e->pix_off[p];
    q.dst_pitch[p] = e->cw[p];
    src[p] = e->d_pix + e->pix_off[p];
    stride[p] = e->cw[p];
  }
  if (a->device) {
    hipStream_t cs = (hipStream_t)a->stream;
    if (!e->ev_conv) ENC_TRY(hipEventCreateWithFlags(&e->ev_conv, hipEventDisableTiming));
    for (int p = 0; p < ns; p++) {
      q.src[p] = a->src[p];
      q.src_pitch[p] = a->pitch[p];
    }
    ENC_TRY(hipEventRecord(e->ev_in, cs));
    ENC_TRY(hipStreamWaitEvent(e->stream, e->ev_in, 0));
    if (thip_picture_in(&q, 1, e->stream)) return TH_EFAULT;
    ENC_TRY(hipEventRecord(e->ev_conv, e->stream));   // the caller's picture has been read
    ENC_TRY(hipStreamWaitEvent(cs, e->ev_conv, 0));
  } else {
    // the previous frame's upload is complete (its packet is out), so the staging buffer is free
    const size_t plane = (size_t)row * a->height;
    const size_t cap = (size_t)4 * a->width * a->height;   // (the largest of the three formats)
    if (!e->h_rgb) ENC_TRY(hipHostMalloc((void **)&e->h_rgb, cap, hipHostMallocDefault));
    if (!e->d_rgb) ENC_TRY(hipMalloc((void **)&e->d_rgb, cap));
    for (int p = 0; p < ns; p++) {
      const uint8_t *in = (const uint8_t *)a->src[p];
      for (int y = 0; y < a->height; y++) memcpy(e->h_rgb + p * plane + (size_t)y * row, in + (int64_t)y * a->pitch[p], (size_t)row);
      q.src[p] = e->d_rgb + p * plane;
      q.src_pitch[p] = row;
    }
    ENC_TRY(hipMemcpyAsync(e->d_rgb, e->h_rgb, ns * plane, hipMemcpyHostToDevice, e->stream));
    if (thip_picture_in(&q, 1, e->stream)) return TH_EFAULT;
  }
  return enc_queue_frame(e, src, stride);
}

static void enc_put_eob_run(std::vector<uint32_t> &m, uint32_t run) {   // token | extra << 5 (a 12-bit run is never 0 here)
  uint32_t t, x;
  if (run <= 3) { t = run - 1; x = 0; }
  else if (run <= 7) { t = 3; x = run - 4; }
  else if (run <= 15) { t = 4; x = run - 8; }
  else if (run <= 31) { t = 5; x = run - 16; }
  else { t = 6; x = run; }
  m.push_back(t | x << 5);
}

// spec 7.3-7.5 of an inter frame: coded flags, macro-block modes, vectors (from h_cmap, h_mb)
static void enc_put_inter_header(th_enc_ctx *e, BitW &bw) {
  // 7.3: super blocks partially coded; of the others, fully coded; the block flags of the partial ones
  std::vector<uint8_t> sbp, sbf, blk;
  for (int sb = 0; sb < e->nsbs; sb++) {
    const int32_t at = e->sb_start[sb], len = e->sb_start[sb + 1] - at;
    int nc = 0;
    for (int32_t k = 0; k < len; k++) nc += e->h_cmap[e->coded_order[at + k]] != 0;
    const bool partial = nc > 0 && nc < len;
    sbp.push_back(partial);
    if (!partial) sbf.push_back(nc == len);
    else
      for (int32_t k = 0; k < len; k++) blk.push_back(e->h_cmap[e->coded_order[at + k]] != 0);
  }
  enc_put_runs(bw, sbp, true);
  enc_put_runs(bw, sbf, true);
  enc_put_runs(bw, blk, false);
  // 7.4: the mode of every macro block with a coded luma block; vectors equal to the last (the one before) become INTER_MV_LAST
  // (INTER_MV_LAST2), with the bookkeeping of 7.5; INTER_MV_FOUR writes its four vectors and makes the last one the last,
  // GOLDEN_MV writes its vector and leaves the bookkeeping alone
  std::vector<uint8_t> modes;
  std::vector<int> mvs;   // the vectors written: x, y
  int lx = 0, ly = 0, l2x = 0, l2y = 0;
  for (const MacroBlock &m : e->mbs) {
    const int32_t mb = m.raster;
    if (!e->h_cmap[m.luma[0]] && !e->h_cmap[m.luma[1]] && !e->h_cmap[m.luma[2]] && !e->h_cmap[m.luma[3]]) {
      e->istats.modes[MODE_INTER_NOMV]++;
      e->mstats.modes[MODE_INTER_NOMV]++;
      continue;
    }
    const uint32_t w = e->modes ? e->h_mb4[mb].x : e->h_mb[mb];
    const int pix = (int)(w & 0xFF);
    int mode = pix == kEncPixIntra ? MODE_INTRA : pix == kEncPixMv ? MODE_INTER_MV : pix == kEncPixGoldNomv ? MODE_GOLDEN_NOMV
             : pix == kEncPixGoldMv ? MODE_GOLDEN_MV : pix == kEncPixFour ? MODE_INTER_MV_FOUR : MODE_INTER_NOMV;
    if (mode == MODE_INTER_MV_FOUR) {
      const uint32_t bw4[2] = {e->h_mb4[mb].y, e->h_mb4[mb].z};
      for (int k = 0; k < 4; k++) {
        const uint32_t v = bw4[k >> 1] >> (16 * (k & 1));
        mvs.push_back((int)(int8_t)v);
        mvs.push_back((int)(int8_t)(v >> 8));
      }
      l2x = lx;
      l2y = ly;
      lx = mvs[mvs.size() - 2];
      ly = mvs[mvs.size() - 1];
    } else if (mode == MODE_GOLDEN_MV) {
      mvs.push_back((int)(int8_t)(w >> 8));
      mvs.push_back((int)(int8_t)(w >> 16));
    } else if (mode == MODE_INTER_MV) {
      const int vx = (int)(int8_t)(w >> 8), vy = (int)(int8_t)(w >> 16);
      if (vx == lx && vy == ly) {
        mode = MODE_INTER_MV_LAST;
      } else if (vx == l2x && vy == l2y) {
        mode = MODE_INTER_MV_LAST2;
        l2x = lx;
        l2y = ly;
        lx = vx;
        ly = vy;
      } else {
        mvs.push_back(vx);
        mvs.push_back(vy);
        l2x = lx;
        l2y = ly;
        lx = vx;
        ly = vy;
      }
    }
    modes.push_back((uint8_t)mode);
    if (mode < 5) e->istats.modes[mode]++;   // (GET_INTER_STATS counts the five modes of the PREV-only coder)
    e->mstats.modes[mode]++;
  }
  e->mstats.vectors = (int32_t)(mvs.size() / 2);
  // the cheapest scheme; scheme 0's alphabet by falling frequency (ties: the lower mode); ties between schemes: the lower index
  int64_t freq[8] = {};
  for (uint8_t m : modes) freq[m]++;
  int alpha0[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  std::stable_sort(alpha0, alpha0 + 8, [&](int a, int b) { return freq[a] > freq[b]; });
  int rank[8][8];   // [scheme][mode] -> code index (scheme 7: none)
  for (int i = 0; i < 8; i++) rank[0][alpha0[i]] = i;
  for (int sc = 1; sc < 7; sc++)
    for (int i = 0; i < 8; i++) rank[sc][kModeAlphabets[sc - 1][i]] = i;
  int scheme = 0;
  int64_t best = -1;
  for (int sc = 0; sc < 8; sc++) {
    int64_t bits = sc == 0 ? 24 : 0;
    for (int m = 0; m < 8; m++) bits += freq[m] * (sc == 7 ? 3 : rank[sc][m] < 7 ? rank[sc][m] + 1 : 7);
    if (best < 0 || bits < best) {
      best = bits;
      scheme = sc;
    }
  }
  bw.put((uint32_t)scheme, 3);
  if (scheme == 0)
    for (int m = 0; m < 8; m++) bw.put((uint32_t)rank[0][m], 3);
  for (uint8_t m : modes) {
    if (scheme == 7) {
      bw.put(m, 3);
    } else {
      const int i = rank[scheme][m];
      bw.put(i < 7 ? ((1u << i) - 1) << 1 : 0x7Fu, i < 7 ? i + 1 : 7);
    }
  }
  e->istats.mode_scheme = scheme;
  // 7.5: the cheaper vector scheme (ties: VLC)
  int64_t vlc = 0;
  for (int v : mvs) vlc += kMvVlc.nbits[v + 31];
  const int mvsch = vlc > 6 * (int64_t)mvs.size() ? 1 : 0;
  bw.put((uint32_t)mvsch, 1);
  for (int v : mvs) enc_put_mv(bw, v, mvsch);
  e->istats.mv_scheme = mvsch;
}

// spec 7.1: the frame's qi list, qis[0] first, each further one behind a 1, a 0 after the last when there are fewer than three
static void enc_put_qis(const th_enc_ctx *e, BitW &bw) {
  bw.put((uint32_t)e->fqis[0], 6);
  for (int k = 1; k < e->fnqis; k++) {
    bw.put(1, 1);
    bw.put((uint32_t)e->fqis[k], 6);
  }
  if (e->fnqis < 3) bw.put(0, 1);
}

// spec 7.6: the qii flags of the coded blocks in coded order (h_qii; every block of a key frame, h_cmap's of an inter frame), as long
// runs: qii > 0 for each, then, with three qis, qii > 1 for those with qii > 0.  Fills e->bstats.
static void enc_put_qiis(th_enc_ctx *e, BitW &bw) {
  thip_enc_block_qi_stats &s = e->bstats;
  memset(&s, 0, sizeof(s));
  s.nqis = e->fnqis;
  for (int k = 0; k < 3; k++) s.qis[k] = k < e->fnqis ? e->fqis[k] : 0;
  std::vector<uint8_t> f1, f2;
  for (int k = 0; k < e->nfrags; k++) {
    const int fi = e->coded_order[k];
    if (!e->frame_key && !e->h_cmap[fi]) continue;
    const int q = e->fnqis > 1 ? e->h_qii[k] : 0, p = fi >= e->fro[2] ? 2 : fi >= e->fro[1] ? 1 : 0;
    s.blocks[q][p]++;
    f1.push_back(q > 0);
    if (q > 0) f2.push_back(q > 1);
  }
  if (e->fnqis < 2) return;
  const int64_t b0 = (int64_t)bw.out->size() * 8 + bw.n;
  enc_put_runs(bw, f1, true);
  if (e->fnqis == 3) enc_put_runs(bw, f2, true);
  s.flag_bits = (int32_t)((int64_t)bw.out->size() * 8 + bw.n - b0);
}

// the frame header in front of the tokens (spec 7.1-7.6) and the statistics that come with it; false: an inter frame with no coded
// block, whose packet is empty
static bool enc_put_frame_header(th_enc_ctx *e, BitW &bw) {
  memset(&e->istats, 0, sizeof(e->istats));
  memset(&e->mstats, 0, sizeof(e->mstats));
  e->istats.mode_scheme = e->istats.mv_scheme = -1;
  if (e->frame_key) {
    e->istats.key = 1;
    e->istats.modes[MODE_INTRA] = e->nmbs;
    e->mstats.modes[MODE_INTRA] = e->nmbs;
    for (int p = 0; p < 3; p++) e->istats.coded[p] = e->nh[p] * e->nv[p];
    bw.put(0, 1);                          // data packet
    bw.put(0, 1);                          // intra frame
    enc_put_qis(e, bw);
    bw.put(0, 3);                          // reserved
    enc_put_qiis(e, bw);
    return true;
  }
  for (int p = 0; p < 3; p++)
    for (int f = e->fro[p]; f < e->fro[p] + e->nh[p] * e->nv[p]; f++) e->istats.coded[p] += e->h_cmap[f] != 0;
  if (!e->istats.coded[0] && !e->istats.coded[1] && !e->istats.coded[2]) return false;
  bw.put(0, 1);                          // data packet
  bw.put(1, 1);                          // inter frame
  enc_put_qis(e, bw);
  enc_put_inter_header(e, bw);
  enc_put_qiis(e, bw);
  return true;
}

// no block coded: the frame is the previous one, a zero-byte packet (what a duplicate is)
static void enc_empty_packet(th_enc_ctx *e) {
  e->pkt.clear();
  e->pkt_data = e->pkt.data();
  e->pkt_size = 0;
  e->stats.tokens = e->stats.tokens_merged = e->stats.bytes = 0;
  for (int c = 0; c < 4; c++) e->stats.huff[c] = -1;
  e->stats.overflow = 0;
  e->stats.qi = e->frame_qi;
  memset(&e->thist, 0, sizeof(e->thist));
  memset(&e->bstats, 0, sizeof(e->bstats));
  enc_mask_stats(e, false);
  enc_roi_stats(e, false);
  enc_rd_stats(e, false);
  enc_skip_stats(e, false);
  enc_rdq_stats(e, false);
}

// the packet of no frame of its own (one the rate controller dropped, a duplicate): empty, and no packer, search or mode choice ran
static void enc_repeat_packet(th_enc_ctx *e, ogg_packet *op) {
  enc_empty_packet(e);
  op->packet = e->pkt.data();
  op->bytes = 0;
  memset(&e->pstats, 0, sizeof(e->pstats));
  e->pstats.fallbacks = e->pack_fallbacks;
  memset(&e->istats, 0, sizeof(e->istats));
  memset(&e->mstats, 0, sizeof(e->mstats));
  e->istats.mode_scheme = e->istats.mv_scheme = -1;
}

// what both packers leave behind: the frame's statistics, the AC tables the next block-qi choice of this frame type counts with, and
// all four tables of an inter packet for the next rate-distortion mode decision
static void enc_packet_done(th_enc_ctx *e, size_t total, size_t merged, const int hti[4], uint32_t overflow, const uint32_t *hist,
                            bool device) {
  memcpy(e->thist.count, hist, sizeof(e->thist.count));   // [5][2][32], the packer's own
  for (int c = 0; c < 4; c++) e->thist.huff[c] = hti[c];
  e->thist.key = e->frame_key ? 1 : 0;
  e->thist.device = device ? 1 : 0;
  if (!e->frame_key)
    for (int c = 0; c < 4; c++) e->rd_hti[c] = hti[c];
  e->bqi_hti[e->frame_key ? 0 : 1][0] = hti[2];
  e->bqi_hti[e->frame_key ? 0 : 1][1] = hti[3];
  e->stats.tokens = (int64_t)total;
  e->stats.tokens_merged = (int64_t)merged;
  e->stats.bytes = (int64_t)e->pkt_size;
  for (int c = 0; c < 4; c++) e->stats.huff[c] = hti[c];
  e->stats.overflow = (int32_t)overflow;
  e->stats.qi = e->frame_qi;
}

// the host packer: the tokens come to the host, which merges the EOB runs, chooses the tables and writes the bits
static int enc_pack_host(th_enc_ctx *e, size_t total, uint32_t overflow) {
  const uint32_t *len = e->h_small;   // [3][64]
  if (total > e->h_tok_cap) {
    if (e->h_tok) (void)hipHostFree(e->h_tok);
    e->h_tok = nullptr;
    e->h_tok_cap = 0;
    const size_t cap = std::max(total + total / 4, (size_t)4096);
    ENC_TRY(hipHostMalloc((void **)&e->h_tok, cap * 4, hipHostMallocDefault));
    e->h_tok_cap = cap;
  }
  if (total) {
    ENC_TRY(hipMemcpyAsync(e->h_tok, e->d_out, total * 4, hipMemcpyDeviceToHost, e->stream));
    ENC_TRY(hipStreamSynchronize(e->stream));
  }
  const double t0 = thip_now();
  // stream order: index z, then plane p; merged lists in the same order, counted per (z, p)
  std::vector<uint32_t> &m = e->merged;
  m.clear();
  m.reserve(total);
  uint32_t mlen[64][3] = {};
  uint32_t run = 0;
  int rz = 0, rp = 0;
  size_t at = 0;
  for (int z = 0; z < 64; z++)
    for (int p = 0; p < 3; p++) {
      const uint32_t nl = len[p * 64 + z];
      for (uint32_t k = 0; k < nl; k++) {
        const uint32_t w = e->h_tok[at++];
        if ((w & 31) == 0) {   // a block's EOB
          if (!run) { rz = z; rp = p; }
          if (++run == 4095) {
            enc_put_eob_run(m, run);
            mlen[rz][rp]++;
            run = 0;
          }
          continue;
        }
        if (run) {
          enc_put_eob_run(m, run);
          mlen[rz][rp]++;
          run = 0;
        }
        m.push_back(w & 0xFFFFu);
        mlen[z][p]++;
      }
    }
  if (run) {
    enc_put_eob_run(m, run);
    mlen[rz][rp]++;
  }
  // per Huffman group and luma / chroma: token counts; the table of least bits for each of the four choices
  uint32_t hist[5][2][32] = {};
  at = 0;
  for (int z = 0; z < 64; z++) {
    const int hg = z == 0 ? 0 : z <= 5 ? 1 : z <= 14 ? 2 : z <= 27 ? 3 : 4;
    for (int p = 0; p < 3; p++)
      for (uint32_t k = 0; k < mlen[z][p]; k++) hist[hg][p > 0][m[at++] & 31]++;
  }
  int hti[4];   // DC luma, DC chroma, AC luma, AC chroma
  for (int c = 0; c < 4; c++) {
    const int ac = c >> 1, ch = c & 1;
    uint64_t best = ~0ull;
    for (int t = 0; t < 16; t++) {
      uint64_t bits = 0;
      for (int hg = ac ? 1 : 0; hg < (ac ? 5 : 1); hg++)
        for (int tok = 0; tok < 32; tok++) bits += (uint64_t)hist[hg][ch][tok] * e->setup.len[16 * hg + t][tok];
      if (bits < best) {
        best = bits;
        hti[c] = t;
      }
    }
  }
  e->pkt.clear();
  e->pkt.reserve(total * 2 + 16);
  BitW bw{&e->pkt};
  if (!enc_put_frame_header(e, bw)) {
    enc_empty_packet(e);
    e->host_ms = (thip_now() - t0) * 1e3;
    return 0;
  }
  const int64_t hbits = (int64_t)e->pkt.size() * 8 + bw.n;
  at = 0;
  for (int z = 0; z < 64; z++) {
    if (z < 2) {
      bw.put((uint32_t)hti[2 * z], 4);
      bw.put((uint32_t)hti[2 * z + 1], 4);
    }
    const int hg = z == 0 ? 0 : z <= 5 ? 1 : z <= 14 ? 2 : z <= 27 ? 3 : 4;
    for (int p = 0; p < 3; p++) {
      const int h = 16 * hg + hti[(z ? 2 : 0) + (p > 0)];
      for (uint32_t k = 0; k < mlen[z][p]; k++) {
        const uint32_t w = m[at++], tok = w & 31;
        bw.put(e->setup.code[h][tok], e->setup.len[h][tok]);
        bw.put(w >> 5, kTokExtraBits[tok]);
      }
    }
  }
  e->pstats.header_bits = hbits;
  e->pstats.token_bits = (int64_t)e->pkt.size() * 8 + bw.n - hbits;
  e->pstats.phase = (int32_t)(hbits & 7);
  bw.flush();
  e->host_ms = (thip_now() - t0) * 1e3;
  e->pkt_data = e->pkt.data();
  e->pkt_size = e->pkt.size();
  enc_packet_done(e, total, m.size(), hti, overflow, &hist[0][0][0], false);
  return overflow ? TH_EFAULT : 0;
}

// the device packetiser's second half (enc_pack_queue queued the first): the host writes the frame header while the device merges,
// chooses and scans; then the bits are placed from bit `phase` = header bits mod 8 of the device's byte 0 and come back behind the
// header's whole bytes in the pinned packet buffer; the header's last partial byte is ORed into the first of them.  The host touches
// the header's bytes only.  A frame whose bits exceed the device buffer goes to the host packer.
static int enc_pack_device(th_enc_ctx *e, size_t total, uint32_t overflow) {
  const double t0 = thip_now();
  double waited = 0;
  e->pkt.clear();
  BitW bw{&e->pkt};
  if (!enc_put_frame_header(e, bw)) {
    enc_empty_packet(e);
    e->host_ms = (thip_now() - t0) * 1e3;
    return 0;
  }
  const size_t hb = e->pkt.size();
  const int phase = bw.n;
  double tw = thip_now();
  ENC_TRY(hipEventSynchronize(e->ev_k1));
  waited += thip_now() - tw;
  float ms = 0;
  const double pack1 = hipEventElapsedTime(&ms, e->ev_k0, e->ev_k1) == hipSuccess ? ms : 0.0;
  const PackRec rec = *e->h_prec;
  const uint64_t need = pack_need_bytes(phase, rec.bits);
  const int capopt = thip_option("enc_pack_cap");
  const uint64_t cap = capopt > 0 ? std::min((uint64_t)capopt, (uint64_t)e->pack_cap) : (uint64_t)e->pack_cap;
  if (rec.total != total) return TH_EFAULT;
  if (!pack_fits(need, cap)) {
    e->pack_fallbacks++;
    const int rc = enc_pack_host(e, total, overflow);
    e->pstats.pack_ms = pack1;
    return rc;
  }
  if (hb + need > e->h_pk_cap) {
    if (e->h_pk) (void)hipHostFree(e->h_pk);
    e->h_pk = nullptr;
    e->h_pk_cap = 0;
    const size_t hcap = std::max((size_t)(hb + need) + (size_t)(hb + need) / 4, (size_t)65536);
    ENC_TRY(hipHostMalloc((void **)&e->h_pk, hcap, hipHostMallocDefault));
    e->h_pk_cap = hcap;
  }
  ENC_TRY(hipEventRecord(e->ev_q0, e->stream));
  ENC_TRY(pack_launch_place(enc_pack_bufs(e), (const uint32_t *)e->d_small, e->pack_groups, phase, e->d_pk, need, e->stream));
  ENC_TRY(hipMemcpyAsync(e->h_pk + hb, e->d_pk, (size_t)need, hipMemcpyDeviceToHost, e->stream));
  ENC_TRY(hipEventRecord(e->ev_q1, e->stream));
  memcpy(e->h_pk, e->pkt.data(), hb);
  tw = thip_now();
  ENC_TRY(hipEventSynchronize(e->ev_q1));
  waited += thip_now() - tw;
  if (phase) e->h_pk[hb] |= (uint8_t)(bw.acc << (8 - phase));
  const double pack2 = hipEventElapsedTime(&ms, e->ev_q0, e->ev_q1) == hipSuccess ? ms : 0.0;
  e->pkt_data = e->h_pk;
  e->pkt_size = hb + (size_t)need;
  e->pstats.device = 1;
  e->pstats.header_bits = (int64_t)hb * 8 + phase;
  e->pstats.token_bits = (int64_t)rec.bits + 16;
  e->pstats.phase = phase;
  e->pstats.pack_ms = pack1 + pack2;
  enc_packet_done(e, total, rec.merged, rec.hti, overflow, (const uint32_t *)(e->h_prec + 1), true);
  e->host_ms = (thip_now() - t0 - waited) * 1e3;   // (the host's own work: the waits for the packetiser are in pack_ms)
  return overflow ? TH_EFAULT : 0;
}

// the packet of the frame queued on the device: the wait for its list lengths, then one of the two packers
static int enc_finish_frame(th_enc_ctx *e) {
  DeviceGuard g(e->device);
  if (enc_2pass_collect(e)) return TH_EFAULT;
  ENC_TRY(hipEventSynchronize(e->ev_done));
  float ms = 0;
  if (hipEventElapsedTime(&ms, e->ev_t0, e->ev_done) == hipSuccess) e->device_ms = ms;
  size_t total = 0;
  for (int k = 0; k < 192; k++) total += e->h_small[k];
  const uint32_t overflow = e->h_small[192];
  if (total > (size_t)e->nfrags * kEncTokWords) return TH_EFAULT;
  memset(&e->pstats, 0, sizeof(e->pstats));
  enc_mask_stats(e, e->mask_queued);   // (an empty packet takes them back)
  enc_roi_stats(e, e->roi_queued);
  enc_rd_stats(e, e->rd_queued);
  enc_skip_stats(e, e->skip_queued);
  enc_rdq_stats(e, e->rdq_queued);
  const int rc = e->frame_dpack ? enc_pack_device(e, total, overflow) : enc_pack_host(e, total, overflow);
  e->pstats.fallbacks = e->pack_fallbacks;
  return rc;
}

static void enc_header(const th_enc_ctx *e, int which, const th_comment *tc, std::vector<uint8_t> &out);

// the reconstruction: the packet just made goes through the encoder's own decoder (created at the first packet, with the encoder's
// headers; no host copy of its pictures); its PREV frame is then the next frame's reference
static int enc_recon(th_enc_ctx *e) {
  if (!e->dec) {
    th_info info;
    th_comment tc;
    th_setup_info *setup = nullptr;
    th_info_init(&info);
    th_comment_init(&tc);
    std::vector<uint8_t> h;
    int rc = 0;
    for (int k = 0; k < 3 && rc >= 0; k++) {
      enc_header(e, k, &tc, h);
      ogg_packet op;
      memset(&op, 0, sizeof(op));
      op.packet = h.data();
      op.bytes = (long)h.size();
      op.b_o_s = k == 0;
      op.packetno = k;
      rc = th_decode_headerin(&info, &tc, &setup, &op);
    }
    if (rc >= 0) e->dec = th_decode_alloc_on(&info, setup, e->device);
    th_setup_free(setup);
    th_comment_clear(&tc);
    th_info_clear(&info);
    if (!e->dec) return TH_EFAULT;
    int off = 0;
    if (th_decode_ctl(e->dec, TH_DECCTL_THIP_SET_HOST_OUTPUT, &off, sizeof(off)) ||
        th_decode_ctl(e->dec, TH_DECCTL_THIP_SET_DEVICE_LISTS, &off, sizeof(off)))
      return TH_EFAULT;
  }
  ogg_packet op;
  memset(&op, 0, sizeof(op));
  op.packet = const_cast<uint8_t *>(e->pkt_data);
  op.bytes = (long)e->pkt_size;
  op.granulepos = -1;
  int64_t gp = 0;
  if (th_decode_packetin(e->dec, &op, &gp) < 0) return TH_EFAULT;
  thip_state *st = thip_dec_backend(e->dec);
  if (!st || thip_state_check_fault(st) < 0) return TH_EFAULT;   // (waits for the decoder's stream)
  e->have_recon = true;
  return 0;
}

static int enc_get_recon(th_enc_ctx *e, th_img_plane *y) {
  if (!e->inter || !e->have_recon) return TH_EINVAL;
  for (int p = 0; p < 3; p++)
    if (y[p].width != e->nh[p] * 8 || y[p].height != e->nv[p] * 8 || !y[p].data || y[p].stride < y[p].width) return TH_EINVAL;
  thip_state *st = thip_dec_backend(e->dec);
  const int prev = st ? thip_state_ref_idx(st, THIP_FRAME_PREV) : -1;
  if (prev < 0) return TH_EFAULT;
  for (int p = 0; p < 3; p++) {
    const int w = y[p].width, h = y[p].height;
    std::vector<uint8_t> tmp((size_t)w * h);
    if (thip_state_read_plane(st, prev, p, tmp.data())) return TH_EFAULT;
    for (int r = 0; r < h; r++) memcpy(y[p].data + (int64_t)r * y[p].stride, tmp.data() + (size_t)(h - 1 - r) * w, (size_t)w);
  }
  return 0;
}

// Quality statistics: the decoder's newest picture over the picture region against the source planes in d_pix, queued on the
// encoder's stream; the metrics go to h_qm.  source: the packet has one (a coded or a dropped frame, not a duplicate).
static int enc_quality_queue(th_enc_ctx *e, bool source) {
  memset(&e->qstats, 0, sizeof(e->qstats));
  e->q_queued = false;
  if (!e->qflags) return 0;
  e->qstats.flags = e->qflags;
  thip_state *st = e->dec ? thip_dec_backend(e->dec) : nullptr;
  if (!source || !e->have_recon || !st) return 0;
  DeviceGuard g(e->device);
  if (!e->d_qm) {
    ENC_TRY(hipMalloc((void **)&e->d_qm, sizeof(thip_picture_metrics)));
    ENC_TRY(hipHostMalloc((void **)&e->h_qm, sizeof(thip_picture_metrics), hipHostMallocDefault));
    ENC_TRY(hipEventCreate(&e->ev_m0));
    ENC_TRY(hipEventCreate(&e->ev_m1));
  }
  thip_picture_compare_req q;
  memset(&q, 0, sizeof(q));
  q.state = st;
  q.bufi = -1;
  q.flags = e->qflags;
  q.x = (int32_t)e->info.pic_x;
  q.y = (int32_t)e->info.pic_y;
  q.width = (int32_t)e->info.pic_width;
  q.height = (int32_t)e->info.pic_height;
  for (int p = 0; p < 3; p++) {
    q.ref[p] = e->d_pix + e->pix_off[p];
    q.ref_pitch[p] = e->cw[p];
  }
  q.result = e->d_qm;
  ENC_TRY(hipEventRecord(e->ev_m0, e->stream));
  if (thip_picture_compare(&q, 1, e->stream)) return TH_EFAULT;
  ENC_TRY(hipEventRecord(e->ev_m1, e->stream));
  ENC_TRY(hipMemcpyAsync(e->h_qm, e->d_qm, sizeof(thip_picture_metrics), hipMemcpyDeviceToHost, e->stream));
  e->qstats.measured = 1;
  e->q_queued = true;
  return 0;
}

static int enc_quality_get(th_enc_ctx *e, thip_enc_quality_stats *out) {
  if (e->q_queued) {
    DeviceGuard g(e->device);
    ENC_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->ev_m0, e->ev_m1) == hipSuccess) e->qstats.compare_ms = ms;
    for (int p = 0; p < 3; p++) {
      e->qstats.sse[p] = e->h_qm->sse[p];
      e->qstats.samples[p] = e->h_qm->samples[p];
      e->qstats.ssim_q20[p] = e->h_qm->ssim_q20[p];
      e->qstats.windows[p] = e->h_qm->windows[p];
    }
    e->q_queued = false;
  }
  *out = e->qstats;
  return 0;
}

int th_encode_packetout(th_enc_ctx *e, int last, ogg_packet *op) {
  if (!e || !op) return TH_EFAULT;
  if (e->done) return 0;
  const int shift = e->info.keyframe_granule_shift;
  int ptype;   // the packet's type in a two-pass record
  if (e->frame_pending && e->rate_dropped) {
    ptype = 3;   // a frame the rate controller dropped: the previous frame again
    e->frame_pending = e->rate_dropped = false;
    ++e->cur;
    e->cstats = e->cnext;
    enc_repeat_packet(e, op);
    const int qrc = enc_quality_queue(e, true);   // (against the picture the decoder goes on showing)
    if (qrc) return qrc;
  } else if (e->frame_pending) {
    e->frame_pending = false;
    const int rc = enc_finish_frame(e);
    if (rc) return rc;
    e->cstats = e->cnext;
    if (e->frame_key) e->key = e->cur + 1;
    ++e->cur;
    if ((e->inter || e->qflags) && e->pkt_size) {
      const int drc = enc_recon(e);
      if (drc) return drc;
    }
    const int qrc = enc_quality_queue(e, true);
    if (qrc) return qrc;
    if (e->twopass.pass == 2) e->twopass.coded(enc_stream(e), e->ratectl, e->frame_key, (int64_t)e->pkt_size * 8);
    else if (e->rate) e->ratectl.coded(enc_stream(e), e->frame_key, (int64_t)e->pkt_size * 8);
    ptype = e->frame_key ? 0 : 1;
    op->packet = const_cast<uint8_t *>(e->pkt_data);
    op->bytes = (long)e->pkt_size;
  } else if (e->dups_left > 0) {
    ptype = 2;
    e->dups_left--;
    ++e->cur;
    if (e->twopass.pass == 2) e->twopass.dup(enc_stream(e), e->ratectl);
    else if (e->rate) e->ratectl.dup(enc_stream(e));
    memset(&e->cstats, 0, sizeof(e->cstats));
    e->cstats.ratio = e->auto_kf;
    enc_repeat_packet(e, op);
    (void)enc_quality_queue(e, false);
  } else {
    return 0;
  }
  op->b_o_s = 0;
  op->e_o_s = last && e->dups_left == 0 ? 1 : 0;
  op->granulepos = ((e->key + e->granpos_bias) << shift) + (e->cur - e->key);
  op->packetno = e->packetno++;
  if (op->e_o_s) e->done = true;
  e->twopass.packet(enc_stream(e), e->ratectl, ptype, e->pkt_size);
  return 1;
}

// header packet `which` (0 info, 1 comment, 2 setup) into out
static void enc_header(const th_enc_ctx *e, int which, const th_comment *tc, std::vector<uint8_t> &out) {
  const th_info &i = e->info;
  out.clear();
  BitW bw{&out};
  bw.put(0x80u + (uint32_t)which, 8);
  for (const char *c = "theora"; *c; c++) bw.put((uint8_t)*c, 8);
  if (which == 0) {   // spec 6.2
    const uint32_t f[][2] = {{3, 8}, {2, 8}, {1, 8}, {i.frame_width >> 4, 16}, {i.frame_height >> 4, 16}, {i.pic_width, 24},
                             {i.pic_height, 24}, {i.pic_x, 8}, {i.frame_height - i.pic_height - i.pic_y, 8},
                             {i.fps_numerator, 32}, {i.fps_denominator, 32}, {i.aspect_numerator, 24},
                             {i.aspect_denominator, 24}, {(uint32_t)i.colorspace, 8}, {(uint32_t)i.target_bitrate, 24}, {(uint32_t)i.quality, 6},
                             {(uint32_t)i.keyframe_granule_shift, 5}, {(uint32_t)i.pixel_fmt, 2}, {0, 3}};
    for (const auto &x : f) bw.put(x[0], (int)x[1]);
  } else if (which == 1) {   // spec 6.3
    auto le32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) bw.put((v >> (8 * k)) & 0xFF, 8); };
    auto bytes = [&](const char *s, uint32_t n) { for (uint32_t k = 0; k < n; k++) bw.put((uint8_t)s[k], 8); };
    const char *vendor = th_version_string();
    le32((uint32_t)strlen(vendor));
    bytes(vendor, (uint32_t)strlen(vendor));
    const int nc = tc->comments > 0 && tc->user_comments ? tc->comments : 0;
    le32((uint32_t)nc);
    for (int k = 0; k < nc; k++) {
      const char *s = tc->user_comments[k] ? tc->user_comments[k] : "";
      const uint32_t n = tc->comment_lengths ? (uint32_t)tc->comment_lengths[k] : (uint32_t)strlen(s);
      le32(n);
      bytes(s, n);
    }
  } else {   // spec 6.4
    const EncSetup &s = e->setup;
    const QuantParams &q = s.qp;
    int nb = 0;
    if (s.custom_quant) {   // a caller's parameters: libtheora's packing, with its duplicate codes (thip_quant.h)
      quant_pack(q, [&](uint32_t v, int n) { bw.put(v, n); });
    } else {
      for (int qi = 0; qi < 64; qi++) nb = std::max(nb, ilog(q.lflims[qi]));
      bw.put((uint32_t)nb, 3);
      for (int qi = 0; qi < 64; qi++) bw.put(q.lflims[qi], nb);
      for (const uint16_t *sc : {q.acscale, q.dcscale}) {
        nb = 1;
        for (int qi = 0; qi < 64; qi++) nb = std::max(nb, ilog(sc[qi]));
        bw.put((uint32_t)nb - 1, 4);
        for (int qi = 0; qi < 64; qi++) bw.put(sc[qi], nb);
      }
      bw.put((uint32_t)q.nbms - 1, 9);
      for (uint8_t b : q.bms) bw.put(b, 8);
      const int bmbits = ilog((uint32_t)q.nbms - 1);
      for (int qti = 0; qti < 2; qti++)
        for (int pli = 0; pli < 3; pli++) {
          if (qti > 0 || pli > 0) bw.put(1, 1);   // NEWQR: every (qti, pli) states its ranges
          bw.put((uint32_t)q.qrbmis[qti][pli][0], bmbits);
          for (int qri = 0, qi = 0; qri < q.nqrs[qti][pli]; qri++) {
            bw.put((uint32_t)q.qrsizes[qti][pli][qri] - 1, ilog((uint32_t)(62 - qi)));
            qi += q.qrsizes[qti][pli][qri];
            bw.put((uint32_t)q.qrbmis[qti][pli][qri + 1], bmbits);
          }
        }
    }
    for (int64_t k = 0; k < s.tree_bits; k++) bw.put((s.trees[k >> 3] >> (7 - (k & 7))) & 1, 1);
  }
  bw.flush();
}

int th_encode_flushheader(th_enc_ctx *e, th_comment *tc, ogg_packet *op) {
  if (!e || !tc || !op) return TH_EFAULT;
  if (e->nheaders_out >= 3) return 0;
  enc_header(e, e->nheaders_out, tc, e->hdr);
  op->packet = e->hdr.data();
  op->bytes = (long)e->hdr.size();
  op->b_o_s = e->nheaders_out == 0;
  op->e_o_s = 0;
  op->granulepos = 0;
  op->packetno = e->packetno++;
  e->nheaders_out++;
  return 1;
}

// a frame has come in: the requests that hold "before the first frame only" are refused from here on
static bool enc_begun(const th_enc_ctx *e) { return e->cur >= 0 || e->frame_pending || e->done; }

int th_encode_ctl(th_enc_ctx *e, int req, void *buf, size_t buf_sz) {
  if (!e) return TH_EFAULT;
  switch (req) {
    case TH_ENCCTL_SET_QUALITY: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (e->rate) return TH_EINVAL;   // (bitrate mode chooses the qi)
      const int q = *(const int *)buf;
      if (q < 0 || q > 63) return TH_EINVAL;
      e->qi = q;
      return 0;
    }
    case TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE: {
      if (!buf || buf_sz != sizeof(uint32_t)) return TH_EINVAL;
      if (!e->inter) {
        *(uint32_t *)buf = 1;   // every frame is a key frame
        return 0;
      }
      const int64_t full = (int64_t)1 << e->info.keyframe_granule_shift;
      e->kf_interval = std::min(std::max((int64_t)*(uint32_t *)buf, (int64_t)1), full);
      *(uint32_t *)buf = (uint32_t)e->kf_interval;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_INTER_FRAMES: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const bool on = *(const int *)buf != 0;
      if (on != e->inter && e->dev_ready) enc_free_device(e);   // (GET_DEVICE made the buffers of the other kind)
      e->inter = on;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_INTER_MODES: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      e->modes = *(const int *)buf != 0;   // (its buffers are made at the first inter frame)
      return 0;
    }
    case TH_ENCCTL_THIP_SET_BLOCK_QI: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const int d = *(const int *)buf;
      if (d < 0 || d > 31) return TH_EINVAL;
      e->bqi = d;   // (its buffers are made at the first frame that uses it)
      return 0;
    }
    case TH_ENCCTL_THIP_SET_MASKING: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const int k = *(const int *)buf;
      if (k != 0 && (k < 2 || k > 16)) return TH_EINVAL;
      e->mask = k;   // (its buffers are made at the first frame that uses it)
      e->kstats.ratio = k;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_ROI_MAP: {
      if (!buf) return TH_EFAULT;
      if (buf_sz != sizeof(thip_enc_roi_map)) return TH_EINVAL;
      const thip_enc_roi_map *a = (const thip_enc_roi_map *)buf;
      if (e->frame_pending || e->done) return TH_EINVAL;
      if (!a->map) {
        e->roi_on = false;   // (its buffers stay)
        e->ostats.active = e->ostats.map_width = e->ostats.map_height = 0;
        return 0;
      }
      if (a->width < 1 || a->width > 16384 || a->height < 1 || a->height > 16384 || (a->device != 0 && a->device != 1)) return TH_EINVAL;
      if ((a->pitch < 0 ? -a->pitch : a->pitch) < a->width) return TH_EINVAL;
      if (!a->device)
        for (int y = 0; y < a->height; y++)
          for (int x = 0; x < a->width; x++) {
            const int v = a->map[(int64_t)y * a->pitch + x];
            if (v < -64 || v > 64) return TH_EINVAL;
          }
      return enc_roi_set(e, a);
    }
    case TH_ENCCTL_THIP_GET_ROI_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_roi_stats)) return TH_EINVAL;
      *(thip_enc_roi_stats *)buf = e->ostats;
      return 0;
    case TH_ENCCTL_THIP_SET_RD_MODES: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const int v = *(const int *)buf;
      if (v != 0 && v != 1) return TH_EINVAL;
      e->rd = v != 0;   // (its buffers are made at the first frame that uses it)
      e->dstats.on = v;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_RD_SKIP: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const int v = *(const int *)buf;
      if (v != 0 && v != 1) return TH_EINVAL;
      e->skip = v != 0;   // (its buffers are made at the first frame that uses it)
      e->sstats.on = v;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_RD_QUANT: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (e->cur >= 0 || e->frame_pending || e->done) return TH_EINVAL;   // before the first frame only
      const int v = *(const int *)buf;
      if (v < 0 || v > 64) return TH_EINVAL;
      e->rdq = v;   // (its buffers are made at the first frame that uses it)
      e->zstats.weight = v;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_DEVICE_PACK: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      const int v = *(const int *)buf;
      if ((v != 0 && v != 1) || e->frame_pending) return TH_EINVAL;
      e->dpack = v != 0;   // (from the next frame on; its buffers are made at the first frame that uses it)
      return 0;
    }
    case TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const int t = *(const int *)buf;
      if (t < 0 || t > 4096) return TH_EINVAL;
      e->auto_kf = t;   // (its buffers are made at the first frame measured)
      e->cstats.ratio = t;
      return 0;
    }
    case TH_ENCCTL_THIP_SET_QUALITY_STATS: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (enc_begun(e)) return TH_EINVAL;
      const int f = *(const int *)buf;
      if (f != 0 && f != THIP_CMP_SSE && f != (THIP_CMP_SSE | THIP_CMP_SSIM)) return TH_EINVAL;
      e->qflags = f;   // (its buffers are made at the first packet measured)
      return 0;
    }
    case TH_ENCCTL_THIP_GET_QUALITY_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_quality_stats)) return TH_EINVAL;
      return enc_quality_get(e, (thip_enc_quality_stats *)buf);
    case TH_ENCCTL_THIP_GET_CUT_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_cut_stats)) return TH_EINVAL;
      *(thip_enc_cut_stats *)buf = e->cstats;
      return 0;
    case TH_ENCCTL_THIP_GET_PACK_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_pack_stats)) return TH_EINVAL;
      *(thip_enc_pack_stats *)buf = e->pstats;
      return 0;
    case TH_ENCCTL_THIP_GET_BLOCK_QI_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_block_qi_stats)) return TH_EINVAL;
      *(thip_enc_block_qi_stats *)buf = e->bstats;
      return 0;
    case TH_ENCCTL_THIP_GET_MASK_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_mask_stats)) return TH_EINVAL;
      *(thip_enc_mask_stats *)buf = e->kstats;
      return 0;
    case TH_ENCCTL_THIP_GET_RD_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_rd_stats)) return TH_EINVAL;
      *(thip_enc_rd_stats *)buf = e->dstats;
      return 0;
    case TH_ENCCTL_THIP_GET_SKIP_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_skip_stats)) return TH_EINVAL;
      *(thip_enc_skip_stats *)buf = e->sstats;
      return 0;
    case TH_ENCCTL_THIP_GET_RD_QUANT_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_rd_quant_stats)) return TH_EINVAL;
      *(thip_enc_rd_quant_stats *)buf = e->zstats;
      return 0;
    case TH_ENCCTL_THIP_2PASS_OUT: {
      if (buf_sz != sizeof(unsigned char *)) return TH_EINVAL;
      if (!buf) return TH_EFAULT;
      if (e->twopass.pass == 2 || (e->twopass.pass == 0 && enc_begun(e))) return TH_EINVAL;   // (the first call)
      return e->twopass.out(enc_stream(e), e->done, (unsigned char **)buf);
    }
    case TH_ENCCTL_THIP_2PASS_IN:
      if (e->twopass.pass == 1 || (e->twopass.pass == 0 && (!e->rate || enc_begun(e)))) return TH_EINVAL;   // (the first call)
      return e->twopass.in(enc_stream(e), (const uint8_t *)buf, buf_sz);
    case TH_ENCCTL_THIP_GET_2PASS_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_2pass_stats)) return TH_EINVAL;
      *(thip_enc_2pass_stats *)buf = e->twopass.stats;
      return 0;
    case TH_ENCCTL_THIP_GET_MODE_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_mode_stats)) return TH_EINVAL;
      *(thip_enc_mode_stats *)buf = e->mstats;
      return 0;
    case TH_ENCCTL_SET_BITRATE: {
      if (!buf) return TH_EINVAL;
      long v;
      if (buf_sz == sizeof(long)) v = *(const long *)buf;
      else if (buf_sz == sizeof(int)) v = *(const int *)buf;
      else return TH_EINVAL;
      if (v < 0) return TH_EINVAL;
      if (v == 0) return TH_EIMPL;   // (leaving bitrate mode)
      e->rate = true;
      if (e->nheaders_out == 0) e->info.target_bitrate = (int)std::min(v, (long)((1 << 24) - 1));
      e->ratectl.set_bitrate(enc_stream(e), (int64_t)v);
      return 0;
    }
    case TH_ENCCTL_SET_RATE_FLAGS:
      if (!e->rate) return TH_EIMPL;
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      e->ratectl.set_flags(*(const int *)buf);
      return 0;
    case TH_ENCCTL_SET_RATE_BUFFER:
      if (!e->rate) return TH_EIMPL;
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      *(int *)buf = e->ratectl.set_buffer(enc_stream(e), *(const int *)buf);
      return 0;
    case TH_ENCCTL_THIP_GET_RATE_STATS:
      if (!e->rate) return TH_EINVAL;
      if (!buf || buf_sz != sizeof(thip_enc_rate_stats)) return TH_EINVAL;
      *(thip_enc_rate_stats *)buf = e->ratectl.stats;
      return 0;
    case TH_ENCCTL_THIP_GET_INTER_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_inter_stats)) return TH_EINVAL;
      *(thip_enc_inter_stats *)buf = e->istats;
      return 0;
    case TH_ENCCTL_THIP_GET_RECON:
      if (!buf || buf_sz != sizeof(th_ycbcr_buffer)) return TH_EINVAL;
      return enc_get_recon(e, (th_img_plane *)buf);
    case TH_ENCCTL_SET_DUP_COUNT: {
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      const int n = *(const int *)buf;
      // the k-th duplicate's granule is ((key + 1) << shift) + k: k must stay below 1 << shift, or it spills into the key frame
      // field (with shift 0 the sum itself counts the frames)
      const int shift = e->info.keyframe_granule_shift;
      if (n < 0 || (shift > 0 && shift < 31 && n >= (1 << shift))) return TH_EINVAL;
      e->dup_next = n;
      return 0;
    }
    case TH_ENCCTL_GET_SPLEVEL_MAX:
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      *(int *)buf = 0;
      return 0;
    case TH_ENCCTL_SET_SPLEVEL:
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      return *(const int *)buf == 0 ? 0 : TH_EINVAL;
    case TH_ENCCTL_THIP_YCBCR_IN_DEVICE:
      if (!buf || buf_sz != sizeof(thip_enc_device_in)) return TH_EINVAL;
      return enc_ycbcr_in_device(e, (const thip_enc_device_in *)buf);
    case TH_ENCCTL_THIP_RGB_IN:
      if (!buf) return TH_EFAULT;
      if (buf_sz != sizeof(thip_enc_rgb_in)) return TH_EINVAL;
      return enc_rgb_in(e, (const thip_enc_rgb_in *)buf);
    case TH_ENCCTL_THIP_GET_DEVICE:
      if (!buf || buf_sz != sizeof(int)) return TH_EINVAL;
      if (!e->dev_ready && enc_ensure_device(e)) return TH_EFAULT;
      *(int *)buf = e->device;
      return 0;
    case TH_ENCCTL_SET_HUFFMAN_CODES: {
      const bool restore = !buf && buf_sz == 0;
      if (!restore && (!buf || buf_sz != sizeof(th_huff_code) * 80 * 32)) return TH_EIMPL;   // (theoraenc_hip.h: the one deviation)
      // every table of code lengths on the device is filled at the first frame that needs it: none exists yet
      if (e->nheaders_out > 0 || enc_begun(e)) return TH_EINVAL;
      if (restore) {
        std::vector<th_huff_code> codes(80 * 32);
        enc_builtin_codes((th_huff_code(*)[32])codes.data());
        enc_setup_codes(e->setup, (const th_huff_code(*)[32])codes.data());
        return 0;
      }
      if (!huff_codes_valid((const th_huff_code(*)[32])buf)) return TH_EINVAL;
      enc_setup_codes(e->setup, (const th_huff_code(*)[32])buf);
      return 0;
    }
    case TH_ENCCTL_SET_QUANT_PARAMS: {
      const bool restore = !buf && buf_sz == 0;
      if (!restore && (!buf || buf_sz != sizeof(th_quant_info))) return TH_EIMPL;   // (theoraenc_hip.h: the deviation of request 0)
      // every table of steps, on the host and on the device, is made at the first frame that needs it: none exists yet
      if (e->nheaders_out > 0 || enc_begun(e)) return TH_EINVAL;
      if (restore) {
        enc_setup_builtin_quant(e->setup);
      } else {
        if (!quant_info_valid((const th_quant_info *)buf)) return TH_EINVAL;
        QuantParams q;
        quant_params_from_info(*(const th_quant_info *)buf, q);   // (before the copy is replaced: buf may be the copy itself)
        e->setup.qp = q;
        e->setup.quant.assign(q);
        e->setup.custom_quant = true;
      }
      enc_setup_lambda(e);
      return 0;
    }
    case TH_ENCCTL_THIP_GET_QUANT_PARAMS:
      if (!buf || buf_sz != sizeof(th_quant_info)) return TH_EINVAL;
      *(th_quant_info *)buf = e->setup.quant.qi;
      return 0;
    case TH_ENCCTL_THIP_GET_HUFFMAN_CODES: {
      if (!buf || buf_sz != sizeof(th_huff_code) * 80 * 32) return TH_EINVAL;
      th_huff_code(*out)[32] = (th_huff_code(*)[32])buf;
      for (int h = 0; h < 80; h++)
        for (int tok = 0; tok < 32; tok++) out[h][tok] = th_huff_code{e->setup.code[h][tok], (int)e->setup.len[h][tok]};
      return 0;
    }
    case TH_ENCCTL_THIP_GET_TOKEN_HIST:
      if (!buf || buf_sz != sizeof(thip_enc_token_hist)) return TH_EINVAL;
      *(thip_enc_token_hist *)buf = e->thist;
      return 0;
    case TH_ENCCTL_THIP_GET_FRAME_STATS:
      if (!buf || buf_sz != sizeof(thip_enc_frame_stats)) return TH_EINVAL;
      *(thip_enc_frame_stats *)buf = e->stats;
      return 0;
    case TH_ENCCTL_THIP_GET_TIMES:
      if (!buf || buf_sz != 2 * sizeof(double)) return TH_EINVAL;
      ((double *)buf)[0] = e->device_ms;
      ((double *)buf)[1] = e->host_ms;
      return 0;
    default: return TH_EIMPL;
  }
}

// the trainer of theoraenc_hip.h's "Huffman codes" (thip_hufftrain.h); start == NULL: the built-in codes
int thip_huff_train(const thip_enc_token_hist *hists, size_t n, const th_huff_code start[80][32], int rounds, th_huff_code out[80][32],
                    thip_huff_train_stats *stats) {
  std::vector<th_huff_code> builtin;
  if (!start) {
    builtin.resize(80 * 32);
    enc_builtin_codes((th_huff_code(*)[32])builtin.data());
    start = (const th_huff_code(*)[32])builtin.data();
  }
  return huff_train(hists, n, start, rounds, out, stats);
}

// the device packetiser on the caller's tokens and tables (theora_hip.h): thip_encode_pack.h's launches, as enc_pack_queue and
// enc_pack_device make them, on the current device's null stream
int thip_enc_pack_tokens(const uint32_t *d_words, const uint32_t list_len[192], const uint32_t codes[80][32], const uint8_t lens[80][32],
                         int groups, int phase, uint8_t *d_packet, size_t cap_bytes, thip_enc_pack_result *res) {
  if (!d_words || !list_len || !codes || !lens || !d_packet || !res) return THIP_EFAULT;
  if (groups < 1 || groups > kPackMaxGroups || phase < 0 || phase > 7 || misaligned(d_packet, 4)) return THIP_EINVAL;
  uint64_t T = 0;
  for (int k = 0; k < 192; k++) T += list_len[k];
  if (T >= (1ull << 31)) return THIP_EINVAL;   // (token indices are 32-bit with room for i + 1)
  if (!table_within(&lens[0][0], 80 * 32, 1, 32)) return THIP_EINVAL;
  std::vector<uint32_t> cl(80 * 32);
  pack_cl_table(cl.data(), lens);
  // one allocation: list_len [192] | hist [320] | codes, cl [80 * 32] | glast [groups] | mtok [T] | gsum, gbase [groups] | rec
  const size_t words = 192 + 320 + 2 * 80 * 32 + (size_t)groups + (size_t)T, words8 = (words + 1) & ~(size_t)1;
  DeviceBuf buf;
  ENC_TRY(buf.alloc(words8 * 4 + 2 * (size_t)groups * sizeof(PackSum) + sizeof(PackRec)));
  uint32_t *w = (uint32_t *)buf.p, *d_len = w;
  PackBufs p;
  p.hist = w + 192;
  p.codes = p.hist + 320;
  p.cl = p.codes + 80 * 32;
  p.glast = p.cl + 80 * 32;
  p.mtok = p.glast + groups;
  p.gsum = (PackSum *)(w + words8);
  p.gbase = p.gsum + groups;
  p.rec = (PackRec *)(p.gbase + groups);
  hipStream_t stream = nullptr;
  ENC_TRY(hipMemcpy(d_len, list_len, 192 * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(p.codes, codes, 80 * 32 * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(p.cl, cl.data(), 80 * 32 * 4, hipMemcpyHostToDevice));
  ENC_TRY(pack_launch_sums(p, d_words, d_len, groups, stream));
  PackRec rec;
  ENC_TRY(hipMemcpy(&rec, p.rec, sizeof(rec), hipMemcpyDeviceToHost));
  if (rec.total != T) return THIP_EFAULT;
  const uint64_t need = pack_need_bytes(phase, rec.bits);
  res->bits = rec.bits;
  res->bytes = need;
  res->tokens = rec.total;
  res->merged = rec.merged;
  res->merged_ac = rec.nac;
  for (int c = 0; c < 4; c++) res->huff[c] = rec.hti[c];
  res->pad = 0;
  if (!pack_fits(need, cap_bytes)) return THIP_ENC_PACK_NOFIT;
  ENC_TRY(pack_launch_place(p, d_len, groups, phase, d_packet, need, stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the inter stage on the caller's planes, lambda and tables (theora_hip.h): the launch functions of thip_rate.h,
// thip_encode_inter.h, thip_encode_modes.h and thip_encode_cut.h, as enc_launch_inter makes them, on the current device's null stream
int thip_enc_inter_stage(const thip_enc_inter_req *q) {
  if (!q) return THIP_EFAULT;
  const int st = q->stages;
  const bool search = st & THIP_ENC_INTER_SEARCH, decide = st & THIP_ENC_INTER_DECIDE, code = st & THIP_ENC_INTER_CODE;
  const bool dconly = st == THIP_ENC_INTER_DC, planes = search || decide || code;
  if (st <= 0 || st > 15 || ((st & THIP_ENC_INTER_DC) && !dconly)) return THIP_EINVAL;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  if (q->classes != 2 && q->classes != 3) return THIP_EINVAL;
  const bool all = q->classes == 3;
  const PicRect pic = pic_rect(*q);
  if (planes) {
    const EntryPlanes pl{q->src, q->src_pitch, q->prev, q->gold, q->ref_pitch};
    if (const int rc = check_picture_planes(f, pic, pl, true, all ? Gold::required : Gold::forbidden)) return rc;
    if ((decide || code) && (q->lambda < 0 || q->lambda > (1 << 24))) return THIP_EINVAL;
    if (search && !q->stats) return THIP_EFAULT;
    if ((decide || code) && !q->words) return THIP_EFAULT;
    if (q->words_from_stats && (!search || !decide || all)) return THIP_EINVAL;
    if (misaligned(q->stats, 16) || misaligned(q->words, all ? 16 : 4) || misaligned(q->words_from_stats, 4)) return THIP_EINVAL;
  }
  if (code) {
    if (!q->dequant) return THIP_EFAULT;
    if (!table_within(q->dequant, 384, 1, 32767)) return THIP_EINVAL;
  }
  if (dconly && (!q->cmap || !q->dcq || !q->dcr)) return THIP_EFAULT;
  if (misaligned(q->levels, 16) || misaligned(q->dcq, 2) || misaligned(q->dcr, 2)) return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int64_t n = geo.nfrags;
  const int classes = q->classes, nmbx = geo.nh[0] >> 1, nmbs = nmbx * (geo.nv[0] >> 1);
  const size_t nchunks = (size_t)((n + kEncChunk - 1) / kEncChunk);
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  const EncRef R = enc_ref(geo, q->prev, q->ref_pitch), G = enc_ref(geo, q->gold, q->ref_pitch);
  hipStream_t stream = nullptr;
  if (search) ENC_TRY(rate_launch_me((uint4 *)q->stats, g, R, nmbx, nmbs, stream));
  if (decide) {
    if (all) ENC_TRY(inter_launch_search((uint4 *)q->words, g, R, G, nmbx, nmbs, q->lambda, stream));
    else ENC_TRY(inter_launch_search((uint32_t *)q->words, g, R, nmbx, nmbs, q->lambda, stream));
    if (q->words_from_stats) ENC_TRY(cut_launch_mb_modes((uint32_t *)q->words_from_stats, (const uint4 *)q->stats, nmbs, q->lambda, stream));
  }
  if (code || dconly) {
    // one allocation: levels [n][64] (when coded and not given) | dclast [chunks][classes] | overflow | order [n] | dequant [384] | dcq, dcr [n] | cmap [n];
    // the outputs the caller gave are used in place of their part
    const size_t o_dclast = code && !q->levels ? (size_t)n * 128 : 0, o_ovf = o_dclast + nchunks * classes * 4, o_order = o_ovf + 16, o_dq = o_order + (size_t)n * 4,
                 o_dcq = o_dq + 768, o_dcr = o_dcq + (((size_t)n * 2 + 15) & ~(size_t)15), o_cmap = o_dcr + (((size_t)n * 2 + 15) & ~(size_t)15);
    DeviceBuf buf;
    ENC_TRY(buf.alloc(o_cmap + (size_t)n));
    uint8_t *const d = buf.p;
    uint32_t *d_dclast = (uint32_t *)(d + o_dclast);
    int16_t *dcq = q->dcq ? q->dcq : (int16_t *)(d + o_dcq), *dcr = q->dcr ? q->dcr : (int16_t *)(d + o_dcr);
    uint8_t *cmap = q->cmap ? q->cmap : d + o_cmap;
    if (code) {
      const InterBufs o{q->levels ? q->levels : (int16_t *)d, dcq, cmap, d_dclast, (uint32_t *)(d + o_ovf)};
      const int32_t *d_order = (const int32_t *)(d + o_order);
      const uint16_t *d_dq = (const uint16_t *)(d + o_dq);
      ENC_TRY(hipMemcpy(d + o_order, geo.coded_order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
      ENC_TRY(hipMemcpy(d + o_dq, q->dequant, 768, hipMemcpyHostToDevice));
      ENC_TRY(hipMemsetAsync(d_dclast, 0, nchunks * classes * 4, stream));
      if (all) ENC_TRY(inter_launch_fq(o, d_order, g, R, G, (const uint4 *)q->words, nmbx, d_dq, n, stream));
      else ENC_TRY(inter_launch_fq(o, d_order, g, R, (const uint32_t *)q->words, nmbx, d_dq, n, stream));
    } else {
      // the last coded fragment (+1) of every 256 fragments and class, formed here as enc_fq_tail's atomicMax leaves it
      std::vector<uint8_t> h_cmap((size_t)n);
      std::vector<uint32_t> h_last(nchunks * classes, 0u);
      ENC_TRY(hipMemcpy(h_cmap.data(), cmap, (size_t)n, hipMemcpyDeviceToHost));
      for (int64_t fi = 0; fi < n; fi++) {
        const int cl = h_cmap[(size_t)fi];
        if (cl > classes) return THIP_EINVAL;
        if (cl) h_last[(size_t)(fi >> 8) * classes + cl - 1] = (uint32_t)fi + 1u;
      }
      ENC_TRY(hipMemcpy(d_dclast, h_last.data(), h_last.size() * 4, hipMemcpyHostToDevice));
    }
    ENC_TRY(hipMemsetAsync(dcr, 0, (size_t)n * 2, stream));   // (the kernel writes the coded fragments' only)
    if (all) ENC_TRY(inter_launch_dc3(dcr, dcq, cmap, d_dclast, g, n, stream));
    else ENC_TRY(inter_launch_dc(dcr, dcq, cmap, d_dclast, g, n, stream));
    ENC_TRY(hipStreamSynchronize(stream));
    return THIP_OK;
  }
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the rate-distortion mode decision on the caller's planes, lambdas and tables (theora_hip.h): thip_encode_rd.h's launch function, as
// enc_rd_queue makes it, on the current device's null stream
int thip_enc_rd_stage(const thip_enc_rd_req *q) {
  if (!q) return THIP_EFAULT;
  const int st = q->stages;
  if (st <= 0 || st > 3) return THIP_EINVAL;
  const bool cand = st & THIP_ENC_RD_CAND, decide = st & THIP_ENC_RD_DECIDE;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  const PicRect pic = pic_rect(*q);
  const EntryPlanes pl{q->src, q->src_pitch, q->prev, q->gold, q->ref_pitch};
  if (const int rc = check_picture_planes(f, pic, pl, true, Gold::required)) return rc;
  if (q->lambda_search < 0 || q->lambda_search > (1 << 24) || q->lambda_rd < 0 || q->lambda_rd > (1 << 24)) return THIP_EINVAL;
  if (!q->cand || (decide && (!q->words || !q->dequant || !q->bits))) return THIP_EFAULT;
  if (decide && !table_within(q->dequant, 384, 1, 32767)) return THIP_EINVAL;
  if (misaligned(q->cand, 16) || misaligned(q->words, 16) || misaligned(q->costs, 8)) return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int nmbx = geo.nh[0] >> 1, nmbs = nmbx * (geo.nv[0] >> 1);
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  const EncRef R = enc_ref(geo, q->prev, q->ref_pitch), G = enc_ref(geo, q->gold, q->ref_pitch);
  // one allocation: dequant [384] | bits [2][5][32]
  DeviceBuf buf;
  ENC_TRY(buf.alloc(768 + 320));
  uint8_t *const d = buf.p;
  if (decide) {
    ENC_TRY(hipMemcpy(d, q->dequant, 768, hipMemcpyHostToDevice));
    ENC_TRY(hipMemcpy(d + 768, q->bits, 320, hipMemcpyHostToDevice));
  }
  hipStream_t stream = nullptr;
  // (the caller's two tables are tables 0 and 1 of the kernel's list: luma, chroma for the DC and the AC groups alike)
  ENC_TRY(rd_launch(RdBufs{(uint4 *)q->cand, (uint4 *)q->words, q->costs}, cand, decide, g, R, G, nmbx, nmbs, q->lambda_search,
                    (int64_t)q->lambda_rd, (const uint16_t *)d, d + 768, make_int4(0, 1, 0, 1), stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the skip decision on the caller's planes, words and tables (theora_hip.h): thip_encode_skip.h's launch function, as enc_skip_queue
// makes it, on the current device's null stream
int thip_enc_skip_stage(const thip_enc_skip_req *q) {
  if (!q) return THIP_EFAULT;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  if (q->classes != 2 && q->classes != 3) return THIP_EINVAL;
  const bool all = q->classes == 3;
  const PicRect pic = pic_rect(*q);
  const EntryPlanes pl{q->src, q->src_pitch, q->prev, q->gold, q->ref_pitch};
  if (const int rc = check_picture_planes(f, pic, pl, true, all ? Gold::required : Gold::forbidden)) return rc;
  if (q->nqis < 1 || q->nqis > 3 || q->lambda < -1 || q->lambda > ((int64_t)1 << 40)) return THIP_EINVAL;
  if (!q->words || !q->dequant || !q->bits) return THIP_EFAULT;
  if (!q->levels || !q->dcq || !q->qii || !q->cmap || !q->skf || !q->dcode || !q->rate || !q->dskip) return THIP_EFAULT;
  if (!table_within(q->dequant, (size_t)q->nqis * 384, 1, 32767) || !table_within(q->bits, 256, 0, 64)) return THIP_EINVAL;
  if (misaligned(q->words, all ? 16 : 4) || misaligned(q->levels, 16) || misaligned(q->dcq, 2) || misaligned(q->iscale, 2) ||
      misaligned(q->dcode, 8) || misaligned(q->rate, 8) || misaligned(q->dskip, 8))
    return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int64_t n = geo.nfrags;
  const int classes = q->classes, nmbx = geo.nh[0] >> 1;
  const size_t nchunks = (size_t)((n + kEncChunk - 1) / kEncChunk);
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  const EncRef R = enc_ref(geo, q->prev, q->ref_pitch), G = enc_ref(geo, all ? q->gold : q->prev, q->ref_pitch);   // (no GOLD: PREV in its place)
  // one allocation: dclast [chunks][classes] | overflow | order [n] | dequant [nqis][384] | bits [256]
  const size_t o_ovf = nchunks * classes * 4, o_order = o_ovf + 16, o_dq = o_order + (size_t)n * 4, o_bits = o_dq + (size_t)q->nqis * 768;
  DeviceBuf buf;
  ENC_TRY(buf.alloc(o_bits + 256));
  uint8_t *const d = buf.p;
  hipStream_t stream = nullptr;
  ENC_TRY(hipMemcpy(d + o_order, geo.coded_order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(d + o_dq, q->dequant, (size_t)q->nqis * 768, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(d + o_bits, q->bits, 256, hipMemcpyHostToDevice));
  ENC_TRY(hipMemsetAsync(d, 0, o_ovf, stream));
  // (the caller's tables are qi 0, 1, 2 of the kernel's table set and AC tables 0, 1 of its bits)
  const InterBufs o{q->levels, q->dcq, q->cmap, (uint32_t *)d, (uint32_t *)(d + o_ovf)};
  const SkipOut so{q->skf, q->dcode, q->rate, q->dskip};
  const BqiSel sel{q->nqis, 0, 1, 2, 0, 1};
  if (all)
    ENC_TRY(skip_launch(o, q->qii, so, (const int32_t *)(d + o_order), g, R, G, (const uint4 *)q->words, nmbx, (const uint16_t *)(d + o_dq),
                        d + o_bits, sel, q->iscale, q->lambda, n, stream));
  else
    ENC_TRY(skip_launch(o, q->qii, so, (const int32_t *)(d + o_order), g, R, G, (const uint32_t *)q->words, nmbx,
                        (const uint16_t *)(d + o_dq), d + o_bits, sel, q->iscale, q->lambda, n, stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the quantising kernels on the caller's planes, words and tables (theora_hip.h): thip_encode_mask.h's launch functions, as
// enc_queue_frame and enc_launch_inter make them, and the DC launch behind an inter frame's, on the current device's null stream
int thip_enc_fq_stage(const thip_enc_fq_req *q) {
  if (!q) return THIP_EFAULT;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  if (q->classes != 0 && q->classes != 2 && q->classes != 3) return THIP_EINVAL;
  const bool all = q->classes == 3, key = q->classes == 0;
  const PicRect pic = pic_rect(*q);
  const EntryPlanes pl{q->src, q->src_pitch, q->prev, q->gold, q->ref_pitch};
  // (a key frame reads no reference: whatever prev and ref_pitch hold is let be)
  if (const int rc = check_picture_planes(f, pic, pl, !key, all ? Gold::required : Gold::forbidden)) return rc;
  if (q->nqis < 0 || q->nqis > 3 || (q->iscale && !q->nqis)) return THIP_EINVAL;
  const int ntabs = key ? 3 : 6, nlist = q->nqis ? q->nqis : 1;
  if (!q->dequant || (q->nqis && (!q->bits || !q->qii)) || !q->levels || !q->dcq || (!key && (!q->words || !q->cmap))) return THIP_EFAULT;
  if (!table_within(q->dequant, (size_t)nlist * ntabs * 64, 1, 32767) || (q->nqis && !table_within(q->bits, 256, 0, 64))) return THIP_EINVAL;
  if ((!key && misaligned(q->words, all ? 16 : 4)) || misaligned(q->levels, 16) || misaligned(q->dcq, 2) || misaligned(q->dcr, 2) ||
      misaligned(q->iscale, 2) || misaligned(q->overflow, 4))
    return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int64_t n = geo.nfrags;
  const int classes = q->classes, nmbx = geo.nh[0] >> 1;
  const size_t nchunks = (size_t)((n + kEncChunk - 1) / kEncChunk);
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  // (a key frame: no planes; no GOLD: PREV in its place)
  const EncRef R = enc_ref(geo, key ? nullptr : q->prev, q->ref_pitch), G = enc_ref(geo, key ? nullptr : all ? q->gold : q->prev, q->ref_pitch);
  // one allocation: dclast [chunks][classes] | overflow | order [n] | dequant [nlist][ntabs][64] | bits [256]
  const size_t dq_bytes = (size_t)nlist * ntabs * 128;
  const size_t o_ovf = nchunks * classes * 4, o_order = o_ovf + 16, o_dq = o_order + (size_t)n * 4, o_bits = o_dq + dq_bytes;
  DeviceBuf buf;
  ENC_TRY(buf.alloc(o_bits + 256));
  uint8_t *const d = buf.p;
  hipStream_t stream = nullptr;
  ENC_TRY(hipMemcpy(d + o_order, geo.coded_order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(d + o_dq, q->dequant, dq_bytes, hipMemcpyHostToDevice));
  if (q->nqis) ENC_TRY(hipMemcpy(d + o_bits, q->bits, 256, hipMemcpyHostToDevice));
  if (o_ovf) ENC_TRY(hipMemsetAsync(d, 0, o_ovf, stream));
  // (the caller's tables are qi 0, 1, 2 of the kernel's table set and AC tables 0, 1 of its bits)
  const BqiSel sel{q->nqis, 0, 1, 2, 0, 1};
  const int32_t *d_order = (const int32_t *)(d + o_order);
  const uint16_t *d_dq = (const uint16_t *)(d + o_dq);
  uint32_t *d_dclast = (uint32_t *)d, *d_ovf = q->overflow ? q->overflow : (uint32_t *)(d + o_ovf);
  if (key) {
    ENC_TRY(fq_launch_key(q->levels, q->dcq, q->qii, d_ovf, d_order, g, d_dq, d + o_bits, sel, q->iscale, n, stream));
  } else {
    const InterBufs o{q->levels, q->dcq, q->cmap, d_dclast, d_ovf};
    if (all) ENC_TRY(fq_launch_inter(o, q->qii, d_order, g, R, G, (const uint4 *)q->words, nmbx, d_dq, d + o_bits, sel, q->iscale, n, stream));
    else ENC_TRY(fq_launch_inter(o, q->qii, d_order, g, R, G, (const uint32_t *)q->words, nmbx, d_dq, d + o_bits, sel, q->iscale, n, stream));
    if (q->dcr) {
      ENC_TRY(hipMemsetAsync(q->dcr, 0, (size_t)n * 2, stream));   // (the kernel writes the coded fragments' only)
      if (all) ENC_TRY(inter_launch_dc3(q->dcr, q->dcq, q->cmap, d_dclast, g, n, stream));
      else ENC_TRY(inter_launch_dc(q->dcr, q->dcq, q->cmap, d_dclast, g, n, stream));
    }
  }
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the level choice on the caller's planes, words, tables and levels (theora_hip.h): thip_encode_rdq.h's launch function, as
// enc_rdq_queue makes it, on the current device's null stream
int thip_enc_rdq_stage(const thip_enc_rdq_req *q) {
  if (!q) return THIP_EFAULT;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  if (q->classes != 0 && q->classes != 2 && q->classes != 3) return THIP_EINVAL;
  const bool all = q->classes == 3, key = q->classes == 0;
  const PicRect pic = pic_rect(*q);
  const EntryPlanes pl{q->src, q->src_pitch, q->prev, q->gold, q->ref_pitch};
  // (a key frame reads no reference: whatever prev, gold and ref_pitch hold is let be)
  if (const int rc = check_picture_planes(f, pic, pl, !key, key ? Gold::ignored : all ? Gold::required : Gold::forbidden)) return rc;
  if (q->nqis < 1 || q->nqis > 3 || q->lambda < -1 || q->lambda > ((int64_t)1 << 40) || q->weight < 0 || q->weight > 64) return THIP_EINVAL;
  if (!q->dequant || !q->bits || !q->levels || (!key && (!q->words || !q->cmap))) return THIP_EFAULT;
  if (!table_within(q->dequant, (size_t)q->nqis * 384, 1, 32767) || !table_within(q->bits, 256, 0, 64)) return THIP_EINVAL;
  if ((!key && misaligned(q->words, all ? 16 : 4)) || misaligned(q->levels, 16) || misaligned(q->iscale, 2) || misaligned(q->jbefore, 8) ||
      misaligned(q->jafter, 8) || misaligned(q->rate, 8))
    return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int64_t n = geo.nfrags;
  const int nmbx = geo.nh[0] >> 1;
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  // (a key frame: no planes; no GOLD: PREV in its place)
  const EncRef R = enc_ref(geo, key ? nullptr : q->prev, q->ref_pitch), G = enc_ref(geo, key ? nullptr : all ? q->gold : q->prev, q->ref_pitch);
  // one allocation: order [n] | dequant [nqis][384] | bits [256]
  const size_t o_dq = (size_t)n * 4, o_bits = o_dq + (size_t)q->nqis * 768;
  DeviceBuf buf;
  ENC_TRY(buf.alloc(o_bits + 256));
  uint8_t *const d = buf.p;
  hipStream_t stream = nullptr;
  ENC_TRY(hipMemcpy(d, geo.coded_order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(d + o_dq, q->dequant, (size_t)q->nqis * 768, hipMemcpyHostToDevice));
  ENC_TRY(hipMemcpy(d + o_bits, q->bits, 256, hipMemcpyHostToDevice));
  // (the caller's tables are qi 0, 1, 2 of the kernel's table set and AC tables 0, 1 of its bits)
  const RdqOut out{q->jbefore, q->jafter, q->rate, nullptr};
  const BqiSel sel{q->nqis, 0, 1, 2, 0, 1};
  if (all)
    ENC_TRY(rdq_launch(3, q->levels, q->qii, q->cmap, out, (const int32_t *)d, g, R, G, (const uint4 *)q->words, nmbx,
                       (const uint16_t *)(d + o_dq), 6, d + o_bits, sel, q->iscale, q->lambda, q->weight, n, stream));
  else
    ENC_TRY(rdq_launch(q->classes, q->levels, q->qii, q->cmap, out, (const int32_t *)d, g, R, G, (const uint32_t *)q->words, nmbx,
                       (const uint16_t *)(d + o_dq), 6, d + o_bits, sel, q->iscale, q->lambda, q->weight, n, stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

int thip_enc_rate_groups(int64_t nfrags) { return nfrags < 1 || nfrags > kRateMaxFrags ? THIP_EINVAL : rate_groups(nfrags); }

// the rate probe's stages on the caller's buffers and tables (theora_hip.h): the launch functions of thip_rate.h, as enc_rate_probe
// makes them, on the current device's null stream
int thip_enc_rate_stage(const thip_enc_rate_req *q) {
  if (!q) return THIP_EFAULT;
  const int st = q->stages;
  if (st <= 0 || st > 15 || (q->inter != 0 && q->inter != 1)) return THIP_EINVAL;
  const bool coef = st & THIP_ENC_RATE_COEF, dc = st & THIP_ENC_RATE_DC, tok = st & THIP_ENC_RATE_TOK, bits = st & THIP_ENC_RATE_BITS;
  const bool inter = q->inter == 1;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt, kRateMaxFrags)) return THIP_EINVAL;
  if (q->groups < 0 || q->groups > rate_groups(kRateMaxFrags)) return THIP_EINVAL;
  const int groups = q->groups ? q->groups : rate_groups(f.nfrags);
  if (rate_blocks_per_group(f.nfrags, groups) >= kRateBlocksPerGroupLimit) return THIP_EINVAL;
  const PicRect pic = pic_rect(*q);
  if (coef) {   // (the one stage that reads pixels: the source's, and PREV's in an inter frame)
    const EntryPlanes pl{q->src, q->src_pitch, q->prev, nullptr, q->ref_pitch};
    if (const int rc = check_picture_planes(f, pic, pl, inter, Gold::ignored)) return rc;
  }
  if ((coef || dc || tok) && (!q->coef || (inter && !q->stats))) return THIP_EFAULT;
  if (dc || tok) {
    if (!q->steps || !q->qdc || (inter && (!q->lambda || !q->coded || !q->cls))) return THIP_EFAULT;
    if (q->any_order != 0 && q->any_order != 1) return THIP_EINVAL;
    if (!rate_steps_ok(q->steps, q->any_order == 1)) return THIP_EINVAL;
    if (inter && !table_within(q->lambda, 64, 0, 1 << 24)) return THIP_EINVAL;
  }
  if ((tok || bits) && !q->partial) return THIP_EFAULT;
  if (bits && (!q->lens || !q->est)) return THIP_EFAULT;
  if (bits && q->fixed < 0) return THIP_EINVAL;
  if (misaligned(q->stats, 16) || misaligned(q->coef, 16) || misaligned(q->qdc, 2) || misaligned(q->coded, 8) || misaligned(q->cls, 8) ||
      misaligned(q->partial, 4) || misaligned(q->est, 8))
    return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int64_t n = geo.nfrags;
  const int nmbx = geo.nh[0] >> 1;
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  const EncRef R = enc_ref(geo, q->prev, q->ref_pitch);
  // one allocation: tab [6][64][64] uint2 | lambda [64] | lens [80][32] | floor [6][64] uint16
  constexpr size_t o_lam = 6 * 64 * 64 * sizeof(uint2), o_lens = o_lam + 64 * sizeof(int), o_floor = o_lens + 80 * 32;
  DeviceBuf buf;
  ENC_TRY(buf.alloc(o_floor + 6 * 64 * sizeof(uint16_t)));
  uint8_t *const d = buf.p;
  if (dc || tok) {
    std::vector<uint2> tab(6 * 64 * 64);
    std::vector<uint16_t> floor(6 * 64);
    rate_form_table(tab.data(), q->steps);
    rate_form_floor(floor.data(), q->steps);
    ENC_TRY(hipMemcpy(d, tab.data(), o_lam, hipMemcpyHostToDevice));
    ENC_TRY(hipMemcpy(d + o_floor, floor.data(), floor.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    if (inter) ENC_TRY(hipMemcpy(d + o_lam, q->lambda, 64 * sizeof(int), hipMemcpyHostToDevice));
  }
  if (bits) ENC_TRY(hipMemcpy(d + o_lens, q->lens, 80 * 32, hipMemcpyHostToDevice));
  RateArgs a;
  a.coef = q->coef;
  a.tab = (const uint2 *)d;
  a.mbs = (const uint4 *)q->stats;
  a.lam = (const int *)(d + o_lam);
  a.floor = (const uint16_t *)(d + o_floor);
  a.nmbx = nmbx;
  a.hdec = geo.hdec;
  a.vdec = geo.vdec;
  hipStream_t stream = nullptr;
  if (coef) {
    if (inter) ENC_TRY(rate_launch_coef(q->coef, g, R, a.mbs, nmbx, n, stream));
    else ENC_TRY(rate_launch_coef(q->coef, g, n, stream));
  }
  if (dc) ENC_TRY(rate_launch_dc(inter, q->qdc, q->coded, q->cls, a, g, n, stream));
  if (tok) ENC_TRY(rate_launch_tok(inter, q->partial, groups, q->qdc, q->coded, q->cls, a, g, n, stream));
  if (bits) ENC_TRY(rate_launch_bits(q->est, q->partial, groups, d + o_lens, q->fixed, stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the masking stage on the caller's planes (theora_hip.h): thip_encode_mask.h's launch functions, as enc_mask_queue makes them, on the
// current device's null stream
int thip_enc_mask_stage(const thip_enc_mask_req *q) {
  if (!q) return THIP_EFAULT;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  const PicRect pic = pic_rect(*q);
  const EntryPlanes pl{q->src, q->src_pitch, nullptr, nullptr, nullptr};
  // (check_picture_planes' three steps, with every NULL pointer refused before any pitch: this entry's order)
  if (pic_outside(pic, f.width, f.height)) return THIP_EINVAL;
  if (const int rc = check_plane_pointers(pl, false, Gold::ignored)) return rc;
  if (!q->act || !q->avg || !q->iscale) return THIP_EFAULT;
  if (pitches_outside(f, pic, pl, false)) return THIP_EINVAL;
  if (q->ratio < 2 || q->ratio > 16) return THIP_EINVAL;
  if (misaligned(q->act, 4) || misaligned(q->avg, 8) || misaligned(q->iscale, 2)) return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const EncPlanes g = enc_planes(geo, pic, q->src, q->src_pitch);
  DeviceBuf buf;
  ENC_TRY(buf.alloc((size_t)mask_parts(f.nluma) * sizeof(MaskPart)));
  MaskPart *const d_part = (MaskPart *)buf.p;
  hipStream_t stream = nullptr;
  ENC_TRY(mask_launch_act(q->act, d_part, g, stream));
  ENC_TRY(mask_launch_scale(q->iscale, (MaskRec *)q->avg, q->act, d_part, g, geo.nfrags, q->ratio, stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the region-of-interest stage on the caller's map (theora_hip.h): thip_encode_roi.h's launch function, as enc_roi_queue makes it, on
// the current device's null stream
int thip_enc_roi_stage(const thip_enc_roi_req *q) {
  if (!q) return THIP_EFAULT;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  const PicRect pic = pic_rect(*q);
  if (pic_outside(pic, f.width, f.height)) return THIP_EINVAL;   // (a picture, and no planes: the kernel reads the map alone)
  if (!q->map || !q->iscale || !q->stats) return THIP_EFAULT;
  if (q->map_width < 1 || q->map_width > 16384 || q->map_height < 1 || q->map_height > 16384) return THIP_EINVAL;
  if ((q->map_pitch < 0 ? -q->map_pitch : q->map_pitch) < q->map_width) return THIP_EINVAL;
  if (misaligned(q->mask_iscale, 2) || misaligned(q->iscale, 2) || misaligned(q->stats, 8)) return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const EncPlanes g = enc_planes(geo, pic, nullptr, nullptr);
  DeviceBuf buf;
  ENC_TRY(buf.alloc((size_t)roi_parts(geo.nfrags) * sizeof(RoiPart)));
  RoiPart *const d_part = (RoiPart *)buf.p;
  hipStream_t stream = nullptr;
  ENC_TRY(roi_launch_scale(q->iscale, q->mask_iscale, d_part, (RoiRec *)q->stats, q->map, q->map_width, q->map_height, q->map_pitch, nullptr,
                           g, geo.nfrags, stream));
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

// the tokeniser on the caller's levels, DCs and map (theora_hip.h): the launch functions of thip_encode.h and thip_encode_inter.h, as
// th_encode_ycbcr_in, enc_launch_inter and enc_queue_tail make them, on the current device's null stream
int thip_enc_tok_stage(const thip_enc_tok_req *q) {
  if (!q) return THIP_EFAULT;
  const int st = q->stages;
  if (st <= 0 || st > 7) return THIP_EINVAL;
  const bool tok = st & THIP_ENC_TOK_TOK, scan = st & THIP_ENC_TOK_SCAN, scatter = st & THIP_ENC_TOK_SCATTER;
  EntryFrame f;
  if (check_frame(f, q->frame_width, q->frame_height, q->pixel_fmt)) return THIP_EINVAL;
  if (q->classes != 0 && q->classes != 2 && q->classes != 3) return THIP_EINVAL;
  const bool inter = q->classes != 0;
  if (tok && (!q->levels || (inter ? !q->dcr || !q->cmap : !q->dcq) || !q->overflow)) return THIP_EFAULT;
  if ((tok || scatter) && (!q->tok || !q->mask)) return THIP_EFAULT;
  if ((tok || scan) && !q->chunk_cnt) return THIP_EFAULT;
  if ((scan || scatter) && (!q->chunk_base || !q->list_len)) return THIP_EFAULT;
  if (scatter && !q->out) return THIP_EFAULT;
  if (misaligned(q->levels, 16) || misaligned(q->dcq, 2) || misaligned(q->dcr, 2) || misaligned(q->mask, 8) || misaligned(q->tok, 4) ||
      misaligned(q->chunk_cnt, 4) || misaligned(q->chunk_base, 4) || misaligned(q->list_len, 4) || misaligned(q->overflow, 4) ||
      misaligned(q->out, 4))
    return THIP_EINVAL;
  // ---- nothing above touched a device ----
  FrameGeometry geo;
  build_geometry(geo, q->frame_width, q->frame_height, q->pixel_fmt);
  const int64_t n = geo.nfrags;
  const size_t nchunks = enc_chunks(n);
  const EncPlanes g = enc_planes(geo, PicRect{}, nullptr, nullptr);   // (the token kernels read the fragment geometry alone: no picture)
  hipStream_t stream = nullptr;
  DeviceBuf buf;   // (order [n], for TOK alone)
  if (tok) {
    ENC_TRY(buf.alloc((size_t)n * 4));
    int32_t *const d_order = (int32_t *)buf.p;
    ENC_TRY(hipMemcpy(d_order, geo.coded_order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    ENC_TRY(hipMemsetAsync(q->overflow, 0, 4, stream));   // (th_encode_*: the quantising kernel zeroes it)
    const TokBufs o{q->tok, q->mask, q->chunk_cnt, q->overflow};
    if (inter) ENC_TRY(tok_launch_inter(o, q->levels, q->dcr, q->cmap, d_order, g, n, stream));
    else ENC_TRY(tok_launch_intra(o, q->levels, q->dcq, d_order, g, n, stream));
  }
  if (scan) ENC_TRY(tok_launch_scan(q->chunk_base, q->list_len, q->chunk_cnt, n, stream));
  if (scatter) {
    // every word the scatter would write lies inside out: the lists' lengths, the chunks' places and the masks read back (th_encode_*
    // sizes its buffer for the worst case and needs none of this)
    std::vector<uint32_t> h_len(192), h_base(nchunks * 64);
    std::vector<uint64_t> h_mask((size_t)n);
    ENC_TRY(hipMemcpy(h_len.data(), q->list_len, 192 * 4, hipMemcpyDeviceToHost));   // (the null stream: behind the launches above)
    ENC_TRY(hipMemcpy(h_base.data(), q->chunk_base, h_base.size() * 4, hipMemcpyDeviceToHost));
    ENC_TRY(hipMemcpy(h_mask.data(), q->mask, (size_t)n * 8, hipMemcpyDeviceToHost));
    uint64_t start[64], total = 0;
    for (int z = 0; z < 64; z++) {
      start[z] = total;
      total += (uint64_t)h_len[z] + h_len[64 + z] + h_len[128 + z];
    }
    if (total > q->out_cap) return THIP_EINVAL;
    for (size_t c = 0; c < nchunks; c++) {
      uint32_t cnt[64] = {};
      for (int64_t k = (int64_t)c * kEncChunk; k < std::min(n, (int64_t)(c + 1) * kEncChunk); k++)
        for (uint64_t m = h_mask[(size_t)k]; m; m &= m - 1) cnt[__builtin_ctzll(m)]++;
      for (int z = 0; z < 64; z++)
        if (cnt[z] && start[z] + h_base[c * 64 + z] + cnt[z] > q->out_cap) return THIP_EINVAL;
    }
    ENC_TRY(tok_launch_scatter(q->out, q->tok, q->mask, q->chunk_base, q->list_len, n, stream));
  }
  ENC_TRY(hipStreamSynchronize(stream));
  return THIP_OK;
}

}  // extern "C"
