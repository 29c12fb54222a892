/* encoder_example_hip.c -- YUV4MPEG2 in, Ogg/Theora out, through this library's intra-only th_encode_* (include/theoraenc_hip.h)
 * and its Ogg writer (include/thip_ogg.h).
 *
 *   encoder_example_hip [-q quality] [-k keyframe_interval [-m] [-a [t]]] [-b delta [--roi x,y,w,h,v]] [-V kbps]
 *                       [--first-pass FILE | --second-pass FILE | --two-pass | --train-huffman] [--quant-from FILE.ogv]
 *                       [-o out.ogv] in.y4m
 *
 * Input: C420jpeg, C420, C420paldv, C420mpeg2 (4:2:0), C422 or C444, any size; no C tag means 4:2:0.  The frame is the picture
 * padded to multiples of 16, the picture region at (0, 0); the picture-size planes go to th_encode_ycbcr_in as they are.  Every
 * frame is a key frame at qi = quality (default 48).  -k: inter frames; -m with it: all eight macro-block modes
 * (TH_ENCCTL_THIP_SET_INTER_MODES: golden-frame prediction, four vectors a macro block); -a with it: a key frame at every scene
 * cut as well, the interval becoming a maximum (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES with the ratio t, 1..4096; 230 without one).  -b: block-level qi with that delta, 1..31
 * (TH_ENCCTL_THIP_SET_BLOCK_QI).  --roi x,y,w,h,v with it: a region of interest (TH_ENCCTL_THIP_SET_ROI_MAP), the rectangle in picture
 * coordinates (y from the top) at importance v, -64..64 in 1/16 octave of lambda, as a map at macro-block resolution: a cell whose
 * top-left pixel lies in the rectangle holds v, the others 0.  --device-pack: the packets' token bits are made on the GPU (TH_ENCCTL_THIP_SET_DEVICE_PACK; the
 * same bytes).  -V: bitrate mode at kbps * 1000 bits a second
 * (TH_ENCCTL_SET_BITRATE), as libtheora's encoder_example -V.  Output on stdout without -o.
 *
 * Two-pass, with libtheora's encoder_example's option names (TH_ENCCTL_THIP_2PASS_OUT / _IN, "Two-pass" in theoraenc_hip.h):
 * --first-pass FILE encodes once, writes the pass file and no video (with -V the first pass runs in bitrate mode, else at -q);
 * --second-pass FILE (needs -V) encodes to that file's curves; --two-pass (needs -V) does both through a temporary file, the first
 * pass at -q, and reads the input twice, so the input must be a file.
 *
 * --train-huffman ("Huffman codes" in theoraenc_hip.h): encodes the input once with the built-in Huffman codes and keeps every
 * packet's token histogram (TH_ENCCTL_THIP_GET_TOKEN_HIST), trains codes on them (thip_huff_train, 8 rounds), and encodes the input
 * again with the trained codes (TH_ENCCTL_SET_HUFFMAN_CODES) into the output.  It reads the input twice too, so the input must be a
 * seekable file; not together with the two-pass options.
 *
 * --quant-from FILE.ogv ("Quantisation parameters" in theoraenc_hip.h): codes with the quantisation parameters of another Ogg/Theora
 * stream -- the first setup header thip_ogg_reader finds in FILE, through thip_quant_info_from_setup and TH_ENCCTL_SET_QUANT_PARAMS.
 * With every other option; both passes of a two-pass encode must be given the same file.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "theoraenc_hip.h"
#include "thip_ogg.h"

static int write_pages(thip_ogg_writer *w, FILE *out) {
  size_t n = 0;
  const unsigned char *p = thip_ogg_writer_pages(w, &n);
  return n && fwrite(p, 1, n, out) != n ? -1 : 0;
}

/* the header line's tags: W, H, F, A, C; 0 on success */
static int parse_header(FILE *in, int *w, int *h, int *fn, int *fd, int *an, int *ad, int *fmt) {
  char line[1024];
  if (!fgets(line, sizeof(line), in) || strncmp(line, "YUV4MPEG2", 9) != 0) return -1;
  *w = *h = 0;
  *fn = 30, *fd = 1, *an = 1, *ad = 1, *fmt = TH_PF_420;
  for (char *t = strtok(line + 9, " \n"); t; t = strtok(NULL, " \n")) {
    switch (t[0]) {
      case 'W': *w = atoi(t + 1); break;
      case 'H': *h = atoi(t + 1); break;
      case 'F': sscanf(t + 1, "%d:%d", fn, fd); break;
      case 'A': sscanf(t + 1, "%d:%d", an, ad); break;
      case 'C':
        if (strncmp(t + 1, "420", 3) == 0) *fmt = TH_PF_420;
        else if (strcmp(t + 1, "422") == 0) *fmt = TH_PF_422;
        else if (strcmp(t + 1, "444") == 0) *fmt = TH_PF_444;
        else return -1;
        break;
      default: break;
    }
  }
  if (*w <= 0 || *h <= 0 || *fn <= 0 || *fd <= 0) return -1;
  if (*an <= 0 || *ad <= 0) *an = *ad = 1;
  return 0;
}

/* one FRAME: 1 read, 0 at the end, -1 on a broken file */
static int read_frame(FILE *in, unsigned char *buf, size_t bytes) {
  char line[256];
  if (!fgets(line, sizeof(line), in)) return 0;
  if (strncmp(line, "FRAME", 5) != 0) return -1;
  return fread(buf, 1, bytes, in) == bytes ? 1 : -1;
}

typedef struct {
  int quality, kf, all_modes, bqi, device_pack, auto_kf;
  long kbps;
  int roi, roi_rect[5];   /* --roi: x, y, w, h, v */
  const th_huff_code (*codes)[TH_NDCT_TOKENS];   /* --train-huffman, the second run: the trained codes (NULL: the built-in ones) */
  struct hist_pool *pool;                        /* ... the first run: every packet's histogram goes here (NULL: none is kept) */
  const th_quant_info *quant;                    /* --quant-from: another stream's quantisation parameters (NULL: the built-in ones) */
} options;

typedef struct hist_pool {
  thip_enc_token_hist *h;
  size_t n, cap;
} hist_pool;

/* the last packet's histogram into the pool; 0 on success */
static int keep_hist(th_enc_ctx *enc, hist_pool *pool) {
  if (pool->n == pool->cap) {
    const size_t cap = pool->cap ? 2 * pool->cap : 64;
    thip_enc_token_hist *h = realloc(pool->h, cap * sizeof(*h));
    if (!h) return -1;
    pool->h = h;
    pool->cap = cap;
  }
  return th_encode_ctl(enc, TH_ENCCTL_THIP_GET_TOKEN_HIST, &pool->h[pool->n++], sizeof(*pool->h));
}

/* feeds the second pass until it can take the next frame (libtheora's encoder_example loop); 0 on success */
static int feed_pass_file(th_enc_ctx *enc, FILE *pf) {
  unsigned char chunk[4096];
  for (;;) {
    const int want = th_encode_ctl(enc, TH_ENCCTL_THIP_2PASS_IN, NULL, 0);
    if (want < 0) return -1;
    if (want == 0) return 0;
    const size_t n = fread(chunk, 1, (size_t)want < sizeof(chunk) ? (size_t)want : sizeof(chunk), pf);
    if (n == 0) return -1;   /* the pass file is shorter than the input */
    const int used = th_encode_ctl(enc, TH_ENCCTL_THIP_2PASS_IN, chunk, n);
    if (used < 0 || (size_t)used != n) return -1;
  }
}

/* one record (or header) of the first pass to the pass file; 0 on success */
static int write_pass_bytes(th_enc_ctx *enc, FILE *pf) {
  unsigned char *p = NULL;
  const int n = th_encode_ctl(enc, TH_ENCCTL_THIP_2PASS_OUT, &p, sizeof(p));
  if (n < 0 || (n > 0 && fwrite(p, 1, (size_t)n, pf) != (size_t)n)) return -1;
  return 0;
}

/* one pass over the input.  pass 0: plain; 1: the first pass, the pass file to pf and no video (out is NULL); 2: the second pass,
   the pass file from pf */
static int encode(const options *o, FILE *in, FILE *out, int pass, FILE *pf) {
  const int quality = o->quality, kf = o->kf;
  int bqi = o->bqi, all_modes = o->all_modes, device_pack = o->device_pack, auto_kf = o->auto_kf;
  const long kbps = o->kbps;
  int w, h, fn, fd, an, ad, fmt;
  if (parse_header(in, &w, &h, &fn, &fd, &an, &ad, &fmt)) {
    fprintf(stderr, "not a YUV4MPEG2 file this example reads\n");
    return 1;
  }
  const int hdec = !(fmt & 1), vdec = !(fmt & 2);
  const int cw = (w + hdec) >> hdec, ch = (h + vdec) >> vdec;
  const size_t ysz = (size_t)w * h, csz = (size_t)cw * ch, fsz = ysz + 2 * csz;

  th_info ti;
  th_info_init(&ti);
  ti.frame_width = (unsigned)(w + 15) & ~15u;
  ti.frame_height = (unsigned)(h + 15) & ~15u;
  ti.pic_width = (unsigned)w;
  ti.pic_height = (unsigned)h;
  ti.pic_x = ti.pic_y = 0;
  ti.fps_numerator = (unsigned)fn;
  ti.fps_denominator = (unsigned)fd;
  ti.aspect_numerator = (unsigned)an;
  ti.aspect_denominator = (unsigned)ad;
  ti.colorspace = TH_CS_UNSPECIFIED;
  ti.pixel_fmt = (th_pixel_fmt)fmt;
  ti.target_bitrate = 0;
  ti.quality = quality;
  ti.keyframe_granule_shift = 6;
  th_enc_ctx *enc = th_encode_alloc(&ti);
  if (!enc) {
    fprintf(stderr, "th_encode_alloc refused the parameters\n");
    return 1;
  }
  if (o->codes && th_encode_ctl(enc, TH_ENCCTL_SET_HUFFMAN_CODES, (void *)o->codes, sizeof(th_huff_code) * TH_NHUFFMAN_TABLES * TH_NDCT_TOKENS)) {
    fprintf(stderr, "Huffman codes refused\n");
    return 1;
  }
  if (o->quant && th_encode_ctl(enc, TH_ENCCTL_SET_QUANT_PARAMS, (void *)o->quant, sizeof(*o->quant))) {
    fprintf(stderr, "quantisation parameters refused\n");
    return 1;
  }
  if (kf > 0) {   /* inter frames, a key frame every kf frames (clamped to 1 << keyframe_granule_shift) */
    int on = 1;
    uint32_t k = (uint32_t)kf;
    if (th_encode_ctl(enc, TH_ENCCTL_THIP_SET_INTER_FRAMES, &on, sizeof(on)) ||
        th_encode_ctl(enc, TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE, &k, sizeof(k))) {
      fprintf(stderr, "inter frames refused\n");
      return 1;
    }
    if (all_modes && th_encode_ctl(enc, TH_ENCCTL_THIP_SET_INTER_MODES, &all_modes, sizeof(all_modes))) {
      fprintf(stderr, "all modes refused\n");
      return 1;
    }
    if (auto_kf && th_encode_ctl(enc, TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, &auto_kf, sizeof(auto_kf))) {
      fprintf(stderr, "automatic key frames refused (ratio 1..4096)\n");
      return 1;
    }
  }
  if (bqi && th_encode_ctl(enc, TH_ENCCTL_THIP_SET_BLOCK_QI, &bqi, sizeof(bqi))) {
    fprintf(stderr, "block qi refused (delta 1..31)\n");
    return 1;
  }
  if (o->roi) {   /* a map at macro-block resolution: v where the cell's top-left pixel lies in the rectangle */
    const int wm = (w + 15) / 16, hm = (h + 15) / 16, *r = o->roi_rect;
    int8_t *map = calloc((size_t)wm * hm, 1);
    for (int cy = 0; map && cy < hm; cy++)
      for (int cx = 0; cx < wm; cx++)
        if (cx * 16 >= r[0] && cx * 16 < r[0] + r[2] && cy * 16 >= r[1] && cy * 16 < r[1] + r[3]) map[cy * wm + cx] = (int8_t)r[4];
    thip_enc_roi_map rm;
    memset(&rm, 0, sizeof(rm));
    rm.width = wm, rm.height = hm, rm.pitch = wm, rm.map = map;
    if (!map || r[4] < -64 || r[4] > 64 || th_encode_ctl(enc, TH_ENCCTL_THIP_SET_ROI_MAP, &rm, sizeof(rm))) {
      fprintf(stderr, "region of interest refused (v -64..64)\n");
      return 1;
    }
    free(map);   /* the encoder has its own copy */
  }
  if (device_pack && th_encode_ctl(enc, TH_ENCCTL_THIP_SET_DEVICE_PACK, &device_pack, sizeof(device_pack))) {
    fprintf(stderr, "device packetiser refused\n");
    return 1;
  }
  if (kbps > 0) {   /* bitrate mode, before the headers so that the info header carries the bitrate */
    long bits = kbps * 1000;
    if (th_encode_ctl(enc, TH_ENCCTL_SET_BITRATE, &bits, sizeof(bits))) {
      fprintf(stderr, "bitrate mode refused\n");
      return 1;
    }
  }
  if (pass == 1 && write_pass_bytes(enc, pf)) {   /* the header's placeholder */
    fprintf(stderr, "first pass refused\n");
    return 1;
  }
  if (pass == 2 && feed_pass_file(enc, pf)) {      /* enters the second pass: the header */
    fprintf(stderr, "second pass refused (not a pass file of this input and these options?)\n");
    return 1;
  }
  thip_ogg_writer *ow = thip_ogg_writer_new(0x7E0u);
  th_comment tc;
  th_comment_init(&tc);
  ogg_packet op;
  int rc = 0;
  while ((rc = th_encode_flushheader(enc, &tc, &op)) > 0)
    if (thip_ogg_writer_packetin(ow, &op)) rc = -1;
  th_comment_clear(&tc);
  thip_ogg_writer_flush(ow);   /* the headers end a page: data starts on a fresh one */
  if (rc < 0 || (out && write_pages(ow, out))) {
    fprintf(stderr, "header error\n");
    return 1;
  }
  unsigned char *buf[2] = {malloc(fsz), malloc(fsz)};
  int cur = 0, have = read_frame(in, buf[0], fsz), nframes = 0;
  while (have == 1) {
    const int next = read_frame(in, buf[cur ^ 1], fsz);   /* one frame ahead: the last packet carries e_o_s */
    if (next < 0) {
      fprintf(stderr, "truncated frame\n");
      return 1;
    }
    th_ycbcr_buffer yb;
    yb[0].width = w, yb[0].height = h, yb[0].stride = w, yb[0].data = buf[cur];
    yb[1].width = cw, yb[1].height = ch, yb[1].stride = cw, yb[1].data = buf[cur] + ysz;
    yb[2].width = cw, yb[2].height = ch, yb[2].stride = cw, yb[2].data = buf[cur] + ysz + csz;
    if (pass == 2 && feed_pass_file(enc, pf)) {
      fprintf(stderr, "the pass file ends before the input\n");
      return 1;
    }
    if (th_encode_ycbcr_in(enc, yb)) {
      fprintf(stderr, "th_encode_ycbcr_in failed\n");
      return 1;
    }
    while ((rc = th_encode_packetout(enc, next == 0, &op)) > 0) {
      if (out && (thip_ogg_writer_packetin(ow, &op) || write_pages(ow, out))) {
        fprintf(stderr, "write error\n");
        return 1;
      }
      if (o->pool && keep_hist(enc, o->pool)) {
        fprintf(stderr, "out of memory\n");
        return 1;
      }
      if (pass == 1 && write_pass_bytes(enc, pf)) {   /* the packet's record */
        fprintf(stderr, "pass file write error\n");
        return 1;
      }
    }
    if (rc < 0) {
      fprintf(stderr, "th_encode_packetout failed (%d)\n", rc);
      return 1;
    }
    nframes++;
    cur ^= 1;
    have = next;
  }
  if (have < 0) {
    fprintf(stderr, "broken YUV4MPEG2 input\n");
    return 1;
  }
  thip_ogg_writer_flush(ow);
  if (out && write_pages(ow, out)) return 1;
  if (pass == 1) {   /* the finished header over the placeholder */
    if (fseek(pf, 0, SEEK_SET) || write_pass_bytes(enc, pf) || fflush(pf)) {
      fprintf(stderr, "pass file write error\n");
      return 1;
    }
  }
  fprintf(stderr, "%d frames%s\n", nframes, pass == 1 ? " (first pass)" : pass == 2 ? " (second pass)" : o->pool ? " (histograms)" : "");
  thip_ogg_writer_free(ow);
  th_encode_free(enc);
  free(buf[0]);
  free(buf[1]);
  return 0;
}

/* the quantisation parameters of the first Theora setup header in an Ogg file ("Quantisation parameters" in theoraenc_hip.h);
   0 on success, qi then owns its arrays (thip_quant_info_free) */
static int quant_from_file(const char *path, th_quant_info *qi) {
  thip_ogg_reader *r = thip_ogg_open_file(path);
  if (!r) return -1;
  ogg_packet op;
  uint32_t serial;
  int rc = -1;
  while (rc && thip_ogg_next_packet(r, &op, &serial) > 0) {
    if (op.bytes < 7 || op.packet[0] != 0x82 || memcmp(op.packet + 1, "theora", 6) != 0) {
      if (op.bytes > 0 && !(op.packet[0] & 0x80)) break;   /* a data packet: the headers are over */
      continue;
    }
    rc = thip_quant_info_from_setup(op.packet, (size_t)op.bytes, qi);
    break;
  }
  thip_ogg_close(r);
  return rc;
}

int main(int argc, char **argv) {
  options o = {48, 0, 0, 0, 0, 0, 0, 0, {0, 0, 0, 0, 0}, NULL, NULL, NULL};
  const char *in_path = NULL, *out_path = NULL, *first = NULL, *second = NULL, *quant_from = NULL;
  int two_pass = 0, train = 0;
  for (int i = 1; i < argc; i++) {
    if (strcmp(argv[i], "-q") == 0 && i + 1 < argc) o.quality = atoi(argv[++i]);
    else if (strcmp(argv[i], "-o") == 0 && i + 1 < argc) out_path = argv[++i];
    else if (strcmp(argv[i], "-k") == 0 && i + 1 < argc) o.kf = atoi(argv[++i]);
    else if (strcmp(argv[i], "-V") == 0 && i + 1 < argc) o.kbps = atol(argv[++i]);
    else if (strcmp(argv[i], "-m") == 0) o.all_modes = 1;
    else if (strcmp(argv[i], "-a") == 0) o.auto_kf = i + 2 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' ? atoi(argv[++i]) : 230;
    else if (strcmp(argv[i], "-b") == 0 && i + 1 < argc) o.bqi = atoi(argv[++i]);
    else if (strcmp(argv[i], "--roi") == 0 && i + 1 < argc)
      o.roi = sscanf(argv[++i], "%d,%d,%d,%d,%d", &o.roi_rect[0], &o.roi_rect[1], &o.roi_rect[2], &o.roi_rect[3], &o.roi_rect[4]) == 5 ? 1 : -1;
    else if (strcmp(argv[i], "--device-pack") == 0) o.device_pack = 1;
    else if (strcmp(argv[i], "--first-pass") == 0 && i + 1 < argc) first = argv[++i];
    else if (strcmp(argv[i], "--second-pass") == 0 && i + 1 < argc) second = argv[++i];
    else if (strcmp(argv[i], "--two-pass") == 0) two_pass = 1;
    else if (strcmp(argv[i], "--train-huffman") == 0) train = 1;
    else if (strcmp(argv[i], "--quant-from") == 0 && i + 1 < argc) quant_from = argv[++i];
    else in_path = argv[i];
  }
  const int npass = (first != NULL) + (second != NULL) + two_pass + train;
  if (!in_path || o.roi < 0 || (o.roi && !o.bqi) || ((o.all_modes || o.auto_kf) && o.kf <= 0) || npass > 1 || ((second || two_pass) && o.kbps <= 0) ||
      ((two_pass || train) && strcmp(in_path, "-") == 0)) {
    fprintf(stderr, "usage: %s [-q quality] [-k keyframe_interval: inter frames [-m: all modes] [-a [t]: key frames at cuts]] [-b delta: block qi [--roi x,y,w,h,v: a region of interest, v in -64..64]] [--device-pack] [-V kbps] [--first-pass FILE | --second-pass FILE (with -V) | --two-pass (with -V; the input a file) | --train-huffman (the input a file)] [--quant-from FILE.ogv: the quantisers of that stream] [-o out.ogv] in.y4m\n", argv[0]);
    return 1;
  }
  static th_quant_info quant;
  if (quant_from) {
    if (quant_from_file(quant_from, &quant)) {
      fprintf(stderr, "no Theora setup header read from %s\n", quant_from);
      return 1;
    }
    o.quant = &quant;
  }
  FILE *in = strcmp(in_path, "-") == 0 ? stdin : fopen(in_path, "rb");
  if (!in) {
    fprintf(stderr, "cannot open %s\n", in_path);
    return 1;
  }
  FILE *pf = NULL;
  if (first || second || two_pass) {
    pf = two_pass ? tmpfile() : fopen(first ? first : second, first ? "wb" : "rb");
    if (!pf) {
      fprintf(stderr, "cannot open the pass file\n");
      return 1;
    }
  }
  if (first) return encode(&o, in, NULL, 1, pf) || fclose(pf) ? 1 : 0;
  if (two_pass) {   /* the first pass at -q, then the input again */
    options p1 = o;
    p1.kbps = 0;
    if (encode(&p1, in, NULL, 1, pf) || fseek(pf, 0, SEEK_SET) || fseek(in, 0, SEEK_SET)) return 1;
  }
  static th_huff_code codes[TH_NHUFFMAN_TABLES][TH_NDCT_TOKENS];
  if (train) {   /* the histograms with the built-in codes, the training, then the input again */
    hist_pool pool = {NULL, 0, 0};
    options p1 = o;
    p1.pool = &pool;
    thip_huff_train_stats st;
    if (fseek(in, 0, SEEK_CUR)) {
      fprintf(stderr, "--train-huffman reads the input twice: it must be a seekable file\n");
      return 1;
    }
    if (encode(&p1, in, NULL, 0, NULL) || fseek(in, 0, SEEK_SET)) return 1;
    if (thip_huff_train(pool.h, pool.n, NULL, 8, codes, &st)) {
      fprintf(stderr, "thip_huff_train failed\n");
      return 1;
    }
    fprintf(stderr, "trained on %zu packets: code bits %llu -> %llu in %d rounds, %d DC and %d AC tables in use\n", pool.n,
            (unsigned long long)st.bits_start, (unsigned long long)st.bits_end, st.rounds, st.dc_tables, st.ac_tables);
    free(pool.h);
    o.codes = (const th_huff_code(*)[TH_NDCT_TOKENS])codes;
  }
  FILE *out = out_path ? fopen(out_path, "wb") : stdout;
  if (!out) {
    fprintf(stderr, "cannot open %s\n", out_path);
    return 1;
  }
  const int rc = encode(&o, in, out, pf ? 2 : 0, pf);
  if (out != stdout) fclose(out);
  if (in != stdin) fclose(in);
  if (pf) fclose(pf);
  thip_quant_info_free(&quant);
  return rc;
}
