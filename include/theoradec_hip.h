/* theoradec_hip.h -- libtheora's decoder API (include/theora/codec.h, theoradec.h) served by
 * the MI355X backend: the same function names, argument meaning and TH_E* return codes, so
 * a program written against libtheoradec relinks against libtheora_hip.so.
 *
 * The structs below restate the PUBLIC layout of the reference's types (they are API
 * facts: codec.h:144-299, theoradec.h:131-215, libogg's ogg_packet); nothing else of the
 * reference is reproduced.  The front end behind these calls -- bit reader, header and
 * frame parsing, Huffman decode, DC un-prediction, token expansion and dequantisation --
 * is written from the Theora specification (doc/spec/spec.tex); the pixel path is the HIP
 * backend of theora_hip.h, driven through the accel-vtable slots exactly where
 * lib/decode.c:2858-2962 drives oc_state_frag_recon / oc_frag_copy_list /
 * oc_state_loop_filter_frag_rows.
 *
 * Not provided (out of scope): the telemetry requests, the legacy theora_* API,
 * th_granule_* helpers beyond th_granule_frame and th_granule_time.  The encoder (intra only) is theoraenc_hip.h.
 */
#ifndef THEORADEC_HIP_H
#define THEORADEC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* codec.h:77-93 */
#define TH_EFAULT (-1)
#define TH_EINVAL (-10)
#define TH_EBADHEADER (-20)
#define TH_ENOTFORMAT (-21)
#define TH_EVERSION (-22)
#define TH_EIMPL (-23)
#define TH_EBADPACKET (-24)
#define TH_DUPFRAME (1)

typedef enum { TH_CS_UNSPECIFIED, TH_CS_ITU_REC_470M, TH_CS_ITU_REC_470BG, TH_CS_NSPACES } th_colorspace;
typedef enum { TH_PF_420, TH_PF_RSVD, TH_PF_422, TH_PF_444, TH_PF_NFORMATS } th_pixel_fmt;

typedef struct {
  int width, height, stride;
  unsigned char *data;
} th_img_plane; /* codec.h:144-153 */
typedef th_img_plane th_ycbcr_buffer[3];

/* A Huffman code of one DCT token (codec.h): the low nbits bits of pattern, the first bit of the code the most significant of
   them.  TH_ENCCTL_SET_HUFFMAN_CODES (theoraenc_hip.h) takes a th_huff_code[TH_NHUFFMAN_TABLES][TH_NDCT_TOKENS]. */
#define TH_NHUFFMAN_TABLES (80)
#define TH_NDCT_TOKENS (32)
typedef struct {
  uint32_t pattern;
  int nbits;
} th_huff_code;

typedef struct { /* codec.h:206-299 */
  unsigned char version_major, version_minor, version_subminor;
  uint32_t frame_width, frame_height;
  uint32_t pic_width, pic_height, pic_x, pic_y;
  uint32_t fps_numerator, fps_denominator;
  uint32_t aspect_numerator, aspect_denominator;
  th_colorspace colorspace;
  th_pixel_fmt pixel_fmt;
  int target_bitrate;
  int quality;
  int keyframe_granule_shift;
} th_info;

typedef struct { /* codec.h:326-335 */
  char **user_comments;
  int *comment_lengths;
  int comments;
  char *vendor;
} th_comment;

/* libogg's ogg_packet (ogg/ogg.h): only packet, bytes and b_o_s are read here. */
typedef struct {
  unsigned char *packet;
  long bytes;
  long b_o_s;
  long e_o_s;
  int64_t granulepos;
  int64_t packetno;
} ogg_packet;

typedef struct th_dec_ctx th_dec_ctx;
typedef struct th_setup_info th_setup_info;

void th_info_init(th_info *info);   /* info.c */
void th_info_clear(th_info *info);
void th_comment_init(th_comment *tc);
void th_comment_clear(th_comment *tc);

/* theoradec.h:234-322 */
int th_decode_headerin(th_info *info, th_comment *tc, th_setup_info **setup, ogg_packet *op);
th_dec_ctx *th_decode_alloc(const th_info *info, const th_setup_info *setup);
/* Extension (not in theoradec.h): the same with the GPU chosen -- device 0 .. thip_device_count()-1 (theora_hip.h), or -1 for
   what th_decode_alloc does: the THIP_DEVICE environment variable if set (a device number, or "rr": the
   contexts of the process take the visible devices in turn), else the calling thread's current device.
   A context stays on its GPU (a single stream is not split); contexts of one process may use all GPUs. */
th_dec_ctx *th_decode_alloc_on(const th_info *info, const th_setup_info *setup, int device);
void th_setup_free(th_setup_info *setup);
int th_decode_ctl(th_dec_ctx *dec, int req, void *buf, size_t buf_sz);
int th_decode_packetin(th_dec_ctx *dec, const ogg_packet *op, int64_t *granpos);
int th_decode_ycbcr_out(th_dec_ctx *dec, th_ycbcr_buffer ycbcr);
void th_decode_free(th_dec_ctx *dec);
int64_t th_granule_frame(void *encdec, int64_t granpos);
double th_granule_time(void *encdec, int64_t granpos);                      /* state.c:1259 */

/* codec.h "Basic shared functions" and comment helpers (internal.c:189-210, info.c) */
const char *th_version_string(void);
uint32_t th_version_number(void);                                          /* bitstream 3.2.1 -> 0x030201 */
int th_packet_isheader(ogg_packet *op);
int th_packet_iskeyframe(ogg_packet *op);                                  /* 1 key, 0 delta (or empty), -1 header */
void th_comment_add(th_comment *tc, const char *comment);
void th_comment_add_tag(th_comment *tc, const char *tag, const char *value);
char *th_comment_query(th_comment *tc, const char *tag, int count);        /* value of the count-th TAG=, or NULL */
int th_comment_query_count(th_comment *tc, const char *tag);

/* th_decode_ctl requests that are honoured (theoradec.h:40-105).  TH_DECCTL_GET_PPLEVEL_MAX answers 7 and
   TH_DECCTL_SET_PPLEVEL takes 0..7 as the reference does (decode.c:32-48, :1989-1997): the de-blocking and
   de-ringing filters of decode.c:1608-1957 run on the GPU (thip_state_postprocess) and th_decode_ycbcr_out
   hands out the post-processed picture; like the reference, a level set between two key frames takes
   effect at the next key frame (decode.c:1221-1223). */
#define TH_DECCTL_GET_PPLEVEL_MAX (1)
#define TH_DECCTL_SET_PPLEVEL (3)
#define TH_DECCTL_SET_GRANPOS (5)
/* theoradec.h:79-92,141-151.  The reference calls back after every few fragment rows while the
   frame is still being decoded; a frame is one batch of GPU work here, so the callback is made
   ONCE per decoded frame, after it is complete and copied to the host, with the whole range of
   fragment rows [0, frame_height/8) -- what the reference's telemetry build does
   (decode.c:2974-2977).  The buffer is the one th_decode_ycbcr_out returns. */
#define TH_DECCTL_SET_STRIPE_CB (7)
typedef void (*th_stripe_decoded_func)(void *ctx, th_ycbcr_buffer buf, int yfrag0, int yfrag_end);
typedef struct {
  void *ctx;
  th_stripe_decoded_func stripe_decoded;
} th_stripe_callback;
/* Extension (not in theoradec.h): a context allocated while THIP_FE_TRACE_BACKEND=1 is set owns no
   device state; th_decode_packetin parses the packet completely and RECORDS the accel-vtable slot
   calls of the frame (state_frag_recon per coded fragment in coded order, frag_copy_list, the loop
   filter limit) instead of making them.  This request fills a thip_slot_trace describing the most
   recent frame (pointers stay valid until the next packet).  It exists so that the host logic can be
   tested without a GPU; on a normal context it returns TH_EINVAL. */
#define TH_DECCTL_THIP_GET_SLOT_TRACE (0x7101)
/* Extension: buf = int.  Non-zero: from the next packet on the DC prediction (spec 7.8, decode.c:1392-1500)
   is undone by the backend on the GPU (thip_state_set_device_dc: an anti-diagonal wavefront per plane)
   instead of by th_decode_packetin on the host; the pictures are the same.  TH_EIMPL for planes of more
   than 1024 fragment rows.  The environment variable THIP_FE_DEVICE_DC=1 sets it for every new context. */
#define TH_DECCTL_THIP_SET_DEVICE_DC (0x7102)
/* Extension: buf = int.  Non-zero: th_decode_packetin only delimits each fragment's DCT tokens; their
   expansion into 64 coefficients and the AC dequantisation (decode.c:1540-1581) happen on the GPU
   (thip_state_frag_recon_tokens / k_expand_tokens), and 4 bytes per non-zero coefficient cross PCIe
   instead of 128 per block.  THIP_FE_DEVICE_TOKENS=1 sets it for every new context. */
#define TH_DECCTL_THIP_SET_DEVICE_TOKENS (0x7103)
/* Extension: buf = int.  Non-zero: th_decode_packetin stops behind the entropy decoder -- the frame's token lists
   (one per plane and zig-zag index, decode.c:993-1139), the coded-fragment list and one word per fragment go to the
   GPU, which finds each fragment's tokens, expands and dequantises them and decodes the frame
   (thip_state_decode_token_lists).  The DC prediction is still undone in th_decode_packetin (a chain through the plane in
   raster order: nanoseconds a fragment on a host core) unless TH_DECCTL_THIP_SET_DEVICE_DC asks for the GPU there too.  Frames with a plane of more than 147456 coded fragments (beyond
   4K) keep the host path.  Zero: the host's own token walk.  Without this call a context follows the option
   fe_device_lists (THIP_FE_DEVICE_LISTS in the environment): 1 / 0, or -1, the default: this path while at most four
   decoder contexts are alive in the process. */
#define TH_DECCTL_THIP_SET_DEVICE_LISTS (0x7104)
/* Extension: buf = ogg_packet (a data packet the caller will hand to th_decode_packetin LATER, announced in decode order).
   What th_decode_packetin reads out of a packet -- coded flags, modes, vectors, qi indices, DCT tokens, and the DC prediction it
   undoes (decode.c:2790-2823 up to the MCU loop) -- depends on the headers and on nothing an earlier frame left behind: only the
   pictures form a chain.  The packet is copied and parsed on a thread of its own (up to option fe_lookahead, default 8, at a
   time); the th_decode_packetin that gets the same bytes adopts the result and does only the hand-over to the GPU, so one
   stream is no longer bound by one host thread.  Returns 0: announced; 1: not taken (no slot free, an empty packet, a context with
   TH_DECCTL_THIP_SET_DEVICE_DC / _DEVICE_TOKENS on, a process confined to one CPU) -- harmless, the packet is parsed in its
   th_decode_packetin as ever.  A th_decode_packetin whose packet is not the oldest announced one drops everything announced and
   parses the ordinary way: announcing is a hint, never a requirement, and the pictures are the same either way.
   (That holds under option fe_pipeline too, include/theora_hip.h -- there th_decode_ycbcr_out hands the oldest announced packet's
   frame to the device before it waits for its own picture: a th_decode_packetin that brings another packet takes that frame back.)

   While a frame is held.  From the th_decode_ycbcr_out(N) that decoded the announced frame N + 1 ahead until the next
   th_decode_packetin, the context holds a frame the caller has not handed in.  Every th_decode_ctl in that interval behaves as if
   frame N were the newest, as it is for the caller and in the reference: a request that changes what the held frame would have
   been TAKES IT BACK first -- reference ring, frame counters, frame type, qi tables, the blocks' qi indices as they were after
   frame N -- once its arguments have been checked, so that a refused request changes nothing; the next th_decode_packetin then
   decodes its packet on the caller's thread like any packet nobody announced (slower for that one frame, always right).  These
   take back: TH_DECCTL_SET_GRANPOS (the counters it sets are frame N's), TH_DECCTL_SET_PPLEVEL with a level above 0 (the held
   frame was decoded unfiltered and untracked), TH_DECCTL_SET_STRIPE_CB (the callback is made inside a frame's
   th_decode_packetin), TH_DECCTL_THIP_SET_DEVICE_DC and _SET_DEVICE_TOKENS, TH_DECCTL_THIP_SET_FRAME_INFO 1 (the held frame was
   decoded without a record).  These leave the held frame alone: every
   TH_DECCTL_GET_*, TH_DECCTL_SET_PPLEVEL 0, TH_DECCTL_THIP_PREFETCH_PACKET, _PICTURE_OUT, _PICTURE_RESIZE, _PICTURE_COMPARE,
   _SET_HOST_OUTPUT, _SET_DEVICE_LISTS, _SET_FRAME_INFO 0, _FRAME_INFO_OUT.
   The picture th_decode_ycbcr_out handed out for frame N stays valid and unchanged either way.  One frame is held at most: the
   backend can take back one (thip_state_ring_rewind, include/theora_hip.h). */
#define TH_DECCTL_THIP_PREFETCH_PACKET (0x7105)
/* Which GPU the context's device state lives on (th_decode_alloc_on, option "device" / THIP_DEVICE): buf = int, receives the
   device index (thip_state_device); TH_EINVAL for a context without device state (slot-trace mode). */
#define TH_DECCTL_THIP_GET_DEVICE (0x7106)
/* Extension: buf = int.  0: decoded frames are no longer copied to the host image one by one as they are decoded (the copy the
   library makes for th_decode_ycbcr_out by default); th_decode_ycbcr_out still works and then copies the picture it is asked for
   on demand.  1 (the default): every frame is copied as it is decoded (unless post-processing replaces the picture, which is
   copied when asked for).  For callers that take their pictures on the device (TH_DECCTL_THIP_PICTURE_OUT). */
#define TH_DECCTL_THIP_SET_HOST_OUTPUT (0x7107)
/* Extension: buf = thip_picture_out_args.  Writes the picture of the frame th_decode_packetin last returned (TH_DUPFRAME: the
   repeated one) to device memory, cropped and converted as thip_picture_out does (include/theora_hip.h: formats THIP_PIC_*,
   chroma THIP_CHROMA_*, the integer colour conversion, alignment, and its ordering and lifetime guarantees): crop 1 = th_info's
   picture region (pic_x, pic_y, pic_width, pic_height), 0 = the whole coded frame; stream = a hipStream_t (NULL: the context's
   own stream, which thip_synchronize waits for); dst on the context's device (TH_DECCTL_THIP_GET_DEVICE).  It is the same
   picture th_decode_ycbcr_out would hand out, also when that call has already decoded the next announced packet ahead (option
   fe_pipeline).  The request itself never decodes ahead and never waits on the host.  Returns 0, what thip_picture_out returns
   for bad arguments, TH_EINVAL before the first frame, TH_EIMPL in slot-trace mode (no device state). */
#define TH_DECCTL_THIP_PICTURE_OUT (0x7108)
typedef struct thip_picture_out_args {
  int32_t format, chroma;  /* THIP_PIC_*, THIP_CHROMA_* */
  int32_t crop;            /* 1: th_info's picture region; 0: the whole coded frame */
  void *dst[3];            /* device memory */
  int64_t dst_pitch[3];    /* bytes per row */
  void *stream;            /* hipStream_t, or NULL */
} thip_picture_out_args;
/* Extension: buf = thip_picture_resize_args.  TH_DECCTL_THIP_PICTURE_OUT at another size: a rectangle of the frame
   th_decode_packetin last returned (TH_DUPFRAME: the repeated one) resampled, converted and written to device memory as
   thip_picture_resize does (include/theora_hip.h: the two filters, the element types, scale and bias, and the limits).  The
   fields are thip_picture_resize_req's without state and bufi; x, y, width, height are display coordinates of the coded frame
   (0 x 0: the whole frame; th_info's picture region is pic_x, pic_y, pic_width, pic_height).  Stream, device, ordering and the
   frame it shows are TH_DECCTL_THIP_PICTURE_OUT's: the request never decodes ahead and never waits on the host.  Returns 0, what
   thip_picture_resize returns for bad arguments, TH_EINVAL before the first frame, TH_EIMPL in slot-trace mode. */
#define TH_DECCTL_THIP_PICTURE_RESIZE (0x7109)
typedef struct thip_picture_resize_args {
  int32_t format, filter, elem;  /* THIP_PIC_*, THIP_FILTER_*, THIP_ELEM_* */
  int32_t x, y, width, height;   /* source rectangle; 0 x 0: the whole coded frame */
  int32_t out_width, out_height;
  float scale[3], bias[3];
  void *dst[3];                  /* device memory */
  int64_t dst_pitch[3];          /* bytes per row */
  void *stream;                  /* hipStream_t, or NULL */
} thip_picture_resize_args;
/* Extension: buf = thip_picture_compare_args.  A rectangle of the frame th_decode_packetin last returned (TH_DUPFRAME: the
   repeated one) compared with a picture in device memory, as thip_picture_compare does (include/theora_hip.h: the planes, the sums,
   the integer SSIM).  The fields are thip_picture_compare_req's without state and bufi; x, y, width, height are display coordinates
   of the coded frame (0 x 0: the whole frame; th_info's picture region is pic_x, pic_y, pic_width, pic_height).  Stream, device,
   ordering and the frame it measures are TH_DECCTL_THIP_PICTURE_RESIZE's: the request never decodes ahead and never waits on the
   host.  Returns 0, what thip_picture_compare returns for bad arguments, TH_EINVAL before the first frame, TH_EIMPL in slot-trace
   mode. */
#define TH_DECCTL_THIP_PICTURE_COMPARE (0x710A)
typedef struct thip_picture_compare_args {
  int32_t flags;                 /* THIP_CMP_SSE | THIP_CMP_SSIM */
  int32_t x, y, width, height;   /* 0 x 0: the whole coded frame */
  const void *ref[3];            /* device memory, rows top first */
  int64_t ref_pitch[3];
  struct thip_picture_metrics *result;  /* (theora_hip.h) device memory, 8-byte aligned */
  uint32_t *block_sse[3];        /* NULL: none */
  int64_t block_pitch[3];
  void *stream;                  /* hipStream_t, or NULL */
} thip_picture_compare_args;
/* Extension: buf = int.  1: from the next packet on the context keeps a record of every frame's side data -- which blocks were
   coded, from which reference, through which vector (thip_state_set_frame_info, include/theora_hip.h: one small launch a frame) --
   for TH_DECCTL_THIP_FRAME_INFO_OUT; a frame held (above) is taken back first.  0 (the default): no record, no launch, no memory;
   a held frame is left alone.  TH_EINVAL in slot-trace mode. */
#define TH_DECCTL_THIP_SET_FRAME_INFO (0x710B)
/* Extension: buf = thip_frame_info_args.  The side data of the frame th_decode_packetin last returned, written to device memory as
   thip_frame_info_out does (include/theora_hip.h: the maps kind, mv and ncoef per plane, the dense field flow, valid; every
   pointer optional).  The fields are thip_frame_info_req's without state and frag_info, plus crop (1: th_info's picture region
   instead of x, y, width, height; 0 x 0 there: the whole coded frame) and stream; the request fills the host fields at the end:
   frame_type, nqis, qis and ncoded (coded fragments) of that frame.  A frame that decoded nothing (TH_DUPFRAME: an empty packet, or
   one with no coded block) reads as every fragment uncoded -- every output zero -- with frame_type 1 (inter), nqis 0 and ncoded 0.
   Stream, device and the frame it describes are TH_DECCTL_THIP_PICTURE_OUT's, also while a frame decoded ahead is held: the request
   never decodes ahead and never waits on the host.  Returns 0, what thip_frame_info_out returns for bad arguments, TH_EINVAL
   before the first packet behind TH_DECCTL_THIP_SET_FRAME_INFO 1 and with the switch off, TH_EIMPL in slot-trace mode. */
#define TH_DECCTL_THIP_FRAME_INFO_OUT (0x710C)
typedef struct thip_frame_info_args {
  int32_t x, y, width, height;   /* display coordinates; 0 x 0: the whole coded frame (ignored with crop) */
  int32_t crop;                  /* 1: th_info's picture region */
  int32_t elem, refs;            /* THIP_ELEM_F16 / _F32 for flow; THIP_FI_REF_* */
  int32_t reserved;
  uint8_t *kind[3];              /* device memory, every pointer optional */
  int64_t kind_pitch[3];         /* bytes per row */
  int8_t *mv[3];
  int64_t mv_pitch[3];
  uint8_t *ncoef[3];
  int64_t ncoef_pitch[3];
  void *flow;
  int64_t flow_pitch;
  uint8_t *valid;
  int64_t valid_pitch;
  void *stream;                  /* hipStream_t, or NULL */
  int32_t frame_type, nqis, qis[3], ncoded;   /* filled by the request (host) */
} thip_frame_info_args;
typedef struct thip_slot_trace {
  int64_t ncoded;           /* state_frag_recon calls, in call (= coded) order */
  const int32_t *fragi;     /* _fragi */
  const uint8_t *pli;       /* _pli */
  const uint8_t *last_zzi;  /* _last_zzi */
  const uint8_t *refi;      /* frags[_fragi].refi */
  const uint16_t *dc_quant; /* _dc_quant */
  const int16_t *mv;        /* frag_mvs[_fragi], OC_MV packing */
  const int16_t *coeffs;    /* _dct_coeffs[0..63] of each call: natural order, AC dequantised, raw DC */
  int64_t nuncoded;         /* fragments handed to frag_copy_list */
  const int64_t *uncoded;
  int32_t flimit;           /* loop_filter_limits[qis[0]] */
  int32_t frame_type;
} thip_slot_trace;

#ifdef __cplusplus
}
#endif
#endif
