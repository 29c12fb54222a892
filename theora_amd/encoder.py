"""Python face of the th_encode_* API exported by libtheora_hip.so (include/theoraenc_hip.h): a Theora encoder whose block work runs
on the GPU, intra-only by default, with motion-compensated inter frames on request (inter=True; all eight macro-block modes with
all_modes=True), at a constant quality or in bitrate mode (bitrate=...), with block-level qi on request (block_qi=delta) and the
packets' token bits made on the GPU on request (device_pack=True), and with key frames at scene cuts on request
(auto_keyframes=True)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OggPacket, ThComment, ThImgPlane, ThInfo, TheoraHipError

TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE = 4
TH_ENCCTL_GET_SPLEVEL_MAX = 12
TH_ENCCTL_SET_SPLEVEL = 14
TH_ENCCTL_SET_DUP_COUNT = 18
TH_ENCCTL_SET_QUALITY = 28
TH_ENCCTL_THIP_YCBCR_IN_DEVICE = 0x7201
TH_ENCCTL_THIP_GET_DEVICE = 0x7202
TH_ENCCTL_THIP_GET_FRAME_STATS = 0x7203
TH_ENCCTL_THIP_GET_TIMES = 0x7204
TH_ENCCTL_THIP_SET_INTER_FRAMES = 0x7205
TH_ENCCTL_THIP_GET_INTER_STATS = 0x7206
TH_ENCCTL_THIP_GET_RECON = 0x7207
TH_ENCCTL_THIP_GET_RATE_STATS = 0x7208
TH_ENCCTL_THIP_SET_INTER_MODES = 0x7209
TH_ENCCTL_THIP_GET_MODE_STATS = 0x720A
TH_ENCCTL_THIP_SET_BLOCK_QI = 0x720B
TH_ENCCTL_THIP_GET_BLOCK_QI_STATS = 0x720C
TH_ENCCTL_THIP_SET_DEVICE_PACK = 0x720D
TH_ENCCTL_THIP_GET_PACK_STATS = 0x720E
TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES = 0x720F
TH_ENCCTL_THIP_GET_CUT_STATS = 0x7210
TH_ENCCTL_THIP_RGB_IN = 0x7211
TH_ENCCTL_THIP_SET_QUALITY_STATS = 0x7212
TH_ENCCTL_THIP_GET_QUALITY_STATS = 0x7213
TH_ENCCTL_THIP_SET_MASKING = 0x7214
TH_ENCCTL_THIP_GET_MASK_STATS = 0x7215
TH_ENCCTL_THIP_SET_RD_MODES = 0x7218
TH_ENCCTL_THIP_GET_RD_STATS = 0x7219
TH_ENCCTL_THIP_2PASS_OUT = 0x721D   # (0x721A is not used)
TH_ENCCTL_THIP_2PASS_IN = 0x721B
TH_ENCCTL_THIP_GET_2PASS_STATS = 0x721C
TH_ENCCTL_THIP_SET_RD_SKIP = 0x721E
TH_ENCCTL_THIP_GET_SKIP_STATS = 0x721F
TH_ENCCTL_THIP_SET_RD_QUANT = 0x7222   # (0x7220 and 0x7221 are not used)
TH_ENCCTL_THIP_GET_RD_QUANT_STATS = 0x7223
TH_ENCCTL_THIP_SET_ROI_MAP = 0x7225   # (0x7224 is not used)
TH_ENCCTL_THIP_GET_ROI_STATS = 0x7226
TH_ENCCTL_THIP_GET_TOKEN_HIST = 0x7227
TH_ENCCTL_THIP_GET_HUFFMAN_CODES = 0x7228
TH_ENCCTL_SET_HUFFMAN_CODES = 0
TH_ENCCTL_SET_QUANT_PARAMS = 2
TH_ENCCTL_THIP_GET_QUANT_PARAMS = 0x7229
TH_NHUFFMAN_TABLES, TH_NDCT_TOKENS = 80, 32
RD_QUANT_DEFAULT = 3   # the recommended weight w (lambda's weight w / 16): include/theoraenc_hip.h, "Level choice"
TWO_PASS_HEADER_BYTES, TWO_PASS_RECORD_BYTES = 1084, 264   # THIP_2PASS_HEADER_BYTES, THIP_2PASS_RECORD_BYTES
RGB_FORMATS = {"rgb": _lib.PIC_RGB24, "rgba": _lib.PIC_RGBA32, "rgb_planar": _lib.PIC_RGB_PLANAR}
AUTO_KEYFRAMES_DEFAULT = 230   # the recommended ratio t (t / 256 = 0.9): include/theoraenc_hip.h, "Automatic key frames"
TH_ENCCTL_SET_RATE_FLAGS = 20
TH_ENCCTL_SET_RATE_BUFFER = 22
TH_ENCCTL_SET_BITRATE = 30
TH_RATECTL_DROP_FRAMES = 1
TH_RATECTL_CAP_OVERFLOW = 2
TH_RATECTL_CAP_UNDERFLOW = 4
MODE_NAMES = ("INTER_NOMV", "INTRA", "INTER_MV", "INTER_MV_LAST", "INTER_MV_LAST2")
ALL_MODE_NAMES = MODE_NAMES + ("GOLDEN_NOMV", "GOLDEN_MV", "INTER_MV_FOUR")


class DeviceIn(C.Structure):
    """thip_enc_device_in (include/theoraenc_hip.h)."""
    _fields_ = [("planes", ThImgPlane * 3), ("stream", C.c_void_p)]


class RgbIn(C.Structure):
    """thip_enc_rgb_in (include/theoraenc_hip.h)."""
    _fields_ = [("format", C.c_int32), ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("src", C.c_void_p * 3), ("pitch", C.c_int64 * 3), ("stream", C.c_void_p)]


class FrameStats(C.Structure):
    """thip_enc_frame_stats (include/theoraenc_hip.h)."""
    _fields_ = [("tokens", C.c_int64), ("tokens_merged", C.c_int64), ("bytes", C.c_int64), ("huff", C.c_int32 * 4),
                ("overflow", C.c_int32), ("qi", C.c_int32)]


class InterStats(C.Structure):
    """thip_enc_inter_stats (include/theoraenc_hip.h)."""
    _fields_ = [("key", C.c_int32), ("modes", C.c_int32 * 5), ("coded", C.c_int32 * 3), ("mode_scheme", C.c_int32),
                ("mv_scheme", C.c_int32)]


class ModeStats(C.Structure):
    """thip_enc_mode_stats (include/theoraenc_hip.h)."""
    _fields_ = [("modes", C.c_int32 * 8), ("vectors", C.c_int32)]


class BlockQiStats(C.Structure):
    """thip_enc_block_qi_stats (include/theoraenc_hip.h)."""
    _fields_ = [("nqis", C.c_int32), ("qis", C.c_int32 * 3), ("blocks", (C.c_int32 * 3) * 3), ("flag_bits", C.c_int32)]


class PackStats(C.Structure):
    """thip_enc_pack_stats (include/theoraenc_hip.h)."""
    _fields_ = [("device", C.c_int32), ("phase", C.c_int32), ("header_bits", C.c_int64), ("token_bits", C.c_int64),
                ("pack_ms", C.c_double), ("fallbacks", C.c_int32), ("reserved", C.c_int32)]


class CutStats(C.Structure):
    """thip_enc_cut_stats (include/theoraenc_hip.h)."""
    _fields_ = [("measured", C.c_int32), ("cut", C.c_int32), ("intra_mbs", C.c_int32), ("ratio", C.c_int32), ("pred", C.c_int64),
                ("intra", C.c_int64), ("measure_ms", C.c_double)]


class QualityStats(C.Structure):
    """thip_enc_quality_stats (include/theoraenc_hip.h)."""
    _fields_ = [("measured", C.c_int32), ("flags", C.c_int32), ("sse", C.c_int64 * 3), ("samples", C.c_int64 * 3),
                ("ssim_q20", C.c_int64 * 3), ("windows", C.c_int64 * 3), ("compare_ms", C.c_double)]


class MaskStats(C.Structure):
    """thip_enc_mask_stats (include/theoraenc_hip.h)."""
    _fields_ = [("ratio", C.c_int32), ("measured", C.c_int32), ("activity_avg", C.c_int64), ("activity_max", C.c_int64),
                ("mask_ms", C.c_double)]


class RoiMap(C.Structure):
    """thip_enc_roi_map (include/theoraenc_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("device", C.c_int32), ("pad", C.c_int32), ("pitch", C.c_int64),
                ("map", C.c_void_p), ("stream", C.c_void_p)]


class RoiStats(C.Structure):
    """thip_enc_roi_stats (include/theoraenc_hip.h)."""
    _fields_ = [("active", C.c_int32), ("measured", C.c_int32), ("map_width", C.c_int32), ("map_height", C.c_int32),
                ("exp_min", C.c_int32), ("exp_max", C.c_int32), ("exp_sum", C.c_int64), ("scale_min", C.c_int32),
                ("scale_max", C.c_int32), ("clamped", C.c_int32), ("reserved", C.c_int32), ("roi_ms", C.c_double)]


class RdStats(C.Structure):
    """thip_enc_rd_stats (include/theoraenc_hip.h)."""
    _fields_ = [("on", C.c_int32), ("measured", C.c_int32), ("huff", C.c_int32 * 4), ("lam", C.c_int64), ("rd_ms", C.c_double)]


class SkipStats(C.Structure):
    """thip_enc_skip_stats (include/theoraenc_hip.h)."""
    _fields_ = [("on", C.c_int32), ("measured", C.c_int32), ("skipped", C.c_int32 * 3), ("demoted", C.c_int32), ("lam", C.c_int64),
                ("skip_ms", C.c_double)]


class RdQuantStats(C.Structure):
    """thip_enc_rd_quant_stats (include/theoraenc_hip.h)."""
    _fields_ = [("weight", C.c_int32), ("measured", C.c_int32), ("zeroed", C.c_int32 * 3), ("lowered", C.c_int32 * 3),
                ("emptied", C.c_int32), ("reserved", C.c_int32), ("rate_before", C.c_int64), ("rate_after", C.c_int64),
                ("dist_before", C.c_int64), ("dist_after", C.c_int64), ("lam", C.c_int64), ("rdq_ms", C.c_double)]


class TwoPassStats(C.Structure):
    """thip_enc_2pass_stats (include/theoraenc_hip.h)."""
    _fields_ = [("pass_", C.c_int32), ("type", C.c_int32), ("frame", C.c_int64), ("qi", C.c_int32), ("reserved", C.c_int32),
                ("recorded", C.c_int64 * 64), ("fresh", C.c_int64 * 64), ("budget_left", C.c_int64), ("recorded_left", C.c_int64),
                ("corr", C.c_int64 * 4), ("wait_ms", C.c_double), ("probe_ms", C.c_double)]


class HuffCode(C.Structure):
    """th_huff_code (include/theoradec_hip.h)."""
    _fields_ = [("pattern", C.c_uint32), ("nbits", C.c_int)]


HuffCodes = (HuffCode * TH_NDCT_TOKENS) * TH_NHUFFMAN_TABLES


class TokenHist(C.Structure):
    """thip_enc_token_hist (include/theoraenc_hip.h)."""
    _fields_ = [("count", ((C.c_uint32 * 32) * 2) * 5), ("huff", C.c_int32 * 4), ("key", C.c_int32), ("device", C.c_int32)]


class HuffTrainStats(C.Structure):
    """thip_huff_train_stats (include/theoraenc_hip.h)."""
    _fields_ = [("bits_start", C.c_uint64), ("bits_end", C.c_uint64), ("rounds", C.c_int32), ("dc_tables", C.c_int32),
                ("ac_tables", C.c_int32), ("samples", C.c_int32)]


def _huff_codes_in(codes):
    """An (80, 32, 2) array of (pattern, nbits) -> th_huff_code[80][32]."""
    a = np.asarray(codes, np.int64)
    if a.shape != (TH_NHUFFMAN_TABLES, TH_NDCT_TOKENS, 2):
        raise ValueError("Huffman codes are an (80, 32, 2) array of (pattern, nbits)")
    if a[..., 0].min() < 0 or a[..., 0].max() >= 1 << 32 or abs(a[..., 1]).max() >= 1 << 31:
        raise ValueError("a pattern is 32 bits wide and nbits an int")
    buf = np.zeros((TH_NHUFFMAN_TABLES, TH_NDCT_TOKENS), np.dtype([("pattern", np.uint32), ("nbits", np.int32)]))
    buf["pattern"], buf["nbits"] = a[..., 0], a[..., 1]
    return HuffCodes.from_buffer_copy(buf.tobytes())


def _huff_codes_out(buf):
    a = np.frombuffer(bytes(buf), np.dtype([("pattern", np.uint32), ("nbits", np.int32)])).reshape(TH_NHUFFMAN_TABLES, TH_NDCT_TOKENS)
    return np.stack([a["pattern"].astype(np.int64), a["nbits"].astype(np.int64)], axis=-1)


class QuantRanges(C.Structure):
    """th_quant_ranges (include/theoraenc_hip.h)."""
    _fields_ = [("nranges", C.c_int), ("sizes", C.POINTER(C.c_int)), ("base_matrices", C.POINTER(C.c_ubyte * 64))]


class QuantInfoStruct(C.Structure):
    """th_quant_info (include/theoraenc_hip.h): 464 bytes."""
    _fields_ = [("dc_scale", C.c_uint16 * 64), ("ac_scale", C.c_uint16 * 64), ("loop_filter_limits", C.c_ubyte * 64),
                ("qi_ranges", (QuantRanges * 3) * 2)]


class QuantInfo:
    """The quantisation parameters of a stream (include/theoraenc_hip.h, "Quantisation parameters"): dc_scale, ac_scale (64 each,
    0..65535), loop_filter_limits (64, 0..127), and per (qti, pli) sizes[qti][pli] (the ranges' sizes, summing to 63) and
    matrices[qti][pli] ((ranges + 1, 64), natural order), all numpy arrays.  struct() builds the th_quant_info and keeps its arrays
    alive with this object."""

    def __init__(self, dc_scale, ac_scale, loop_filter_limits, sizes, matrices):
        self.dc_scale = np.asarray(dc_scale, np.int64).reshape(64)
        self.ac_scale = np.asarray(ac_scale, np.int64).reshape(64)
        self.loop_filter_limits = np.asarray(loop_filter_limits, np.int64).reshape(64)
        self.sizes = [[np.asarray(sizes[qti][pli], np.int64).reshape(-1) for pli in range(3)] for qti in range(2)]
        self.matrices = [[np.asarray(matrices[qti][pli], np.int64).reshape(-1, 64) for pli in range(3)] for qti in range(2)]
        self._keep = None

    def struct(self):
        """-> th_quant_info as the arrays are now (no check beyond the widths of the fields: the library checks validity)."""
        for a, top in ((self.dc_scale, 65535), (self.ac_scale, 65535), (self.loop_filter_limits, 255)):
            if a.min() < 0 or a.max() > top:
                raise ValueError("a scale is 16 bits wide and a loop-filter limit 8")
        s, keep = QuantInfoStruct(), []
        s.dc_scale[:], s.ac_scale[:] = [int(v) for v in self.dc_scale], [int(v) for v in self.ac_scale]
        s.loop_filter_limits[:] = [int(v) for v in self.loop_filter_limits]
        for qti in range(2):
            for pli in range(3):
                sz, m = self.sizes[qti][pli], self.matrices[qti][pli]
                if len(m) != len(sz) + 1 or (m.size and (m.min() < 0 or m.max() > 255)) or (sz.size and abs(sz).max() >= 1 << 31):
                    raise ValueError("(qti %d, pli %d): n sizes go with n + 1 matrices of 64 bytes" % (qti, pli))
                csz = (C.c_int * max(len(sz), 1))(*[int(v) for v in sz])
                cm = ((C.c_ubyte * 64) * len(m)).from_buffer_copy(m.astype(np.uint8).tobytes())
                keep += [csz, cm]
                r = s.qi_ranges[qti][pli]
                r.nranges, r.sizes, r.base_matrices = len(sz), csz, C.cast(cm, C.POINTER(C.c_ubyte * 64))
        self._keep = (s, keep)
        return s

    @classmethod
    def from_struct(cls, s):
        """A th_quant_info -> QuantInfo (copies everything: the struct's arrays may go away)."""
        sizes, mats = [[None] * 3 for _ in range(2)], [[None] * 3 for _ in range(2)]
        for qti in range(2):
            for pli in range(3):
                r = s.qi_ranges[qti][pli]
                sizes[qti][pli] = np.array([r.sizes[k] for k in range(r.nranges)], np.int64)
                mats[qti][pli] = np.array([list(r.base_matrices[k]) for k in range(r.nranges + 1)], np.int64).reshape(-1, 64)
        return cls(list(s.dc_scale), list(s.ac_scale), list(s.loop_filter_limits), sizes, mats)

    def __eq__(self, o):
        return (isinstance(o, QuantInfo) and np.array_equal(self.dc_scale, o.dc_scale) and np.array_equal(self.ac_scale, o.ac_scale)
                and np.array_equal(self.loop_filter_limits, o.loop_filter_limits)
                and all(np.array_equal(self.sizes[t][p], o.sizes[t][p]) and np.array_equal(self.matrices[t][p], o.matrices[t][p])
                        for t in range(2) for p in range(3)))

    __hash__ = None


def quant_from_setup(packet):
    """thip_quant_info_from_setup: the quantisation parameters of a Theora setup header packet -> QuantInfo.  ValueError for bytes
    th_decode_headerin refuses as a setup header.  Host only."""
    L = _lib.load()
    s = QuantInfoStruct()
    data = bytes(packet)
    rc = L.thip_quant_info_from_setup(data, len(data), C.byref(s))
    if rc < 0:
        raise ValueError("thip_quant_info_from_setup returned %d" % rc)
    try:
        return QuantInfo.from_struct(s)
    finally:
        L.thip_quant_info_free(C.byref(s))


def quant_from_headers(header_packets):
    """The quantisation parameters of a stream from its header packets (the setup header is the one of type 0x82) -> QuantInfo,
    for Encoder(quant=...)."""
    for pkt in header_packets:
        if len(pkt) and bytes(pkt)[0] == 0x82:
            return quant_from_setup(pkt)
    raise ValueError("no setup header among the packets")


def _token_hist_dict(h):
    return dict(count=np.frombuffer(bytes(h.count), np.uint32).reshape(5, 2, 32).astype(np.int64), huff=list(h.huff), key=int(h.key),
                device=int(h.device))


def train_huffman(hists, start=None, rounds=8):
    """thip_huff_train (include/theoraenc_hip.h, "Huffman codes"): codes trained on the packets' token histograms, from `start`
    (None: the built-in codes) -> (codes, stats).  hists: Encoder.token_hist() dicts, or (5, 2, 32) count arrays.  codes is an
    (80, 32, 2) array of (pattern, nbits) for Encoder(huffman=...); stats has bits_start, bits_end, rounds, dc_tables, ac_tables,
    samples.  Host arithmetic: no GPU."""
    L = _lib.load()
    hists = list(hists)
    arr = (TokenHist * max(len(hists), 1))()
    for k, h in enumerate(hists):
        cnt = np.asarray(h["count"] if isinstance(h, dict) else h, np.int64)
        if cnt.shape != (5, 2, 32) or cnt.min() < 0 or cnt.max() >= 1 << 32:
            raise ValueError("a histogram is a (5, 2, 32) array of 32-bit counts")
        C.memmove(arr[k].count, cnt.astype(np.uint32).tobytes(), 5 * 2 * 32 * 4)
    out, st = HuffCodes(), HuffTrainStats()
    rc = L.thip_huff_train(arr if hists else None, len(hists), None if start is None else _huff_codes_in(start), int(rounds), out,
                           C.byref(st))
    if rc < 0:
        raise ValueError("thip_huff_train returned %d (rounds 1..64, at most 2^20 histograms, a valid start)" % rc)
    return _huff_codes_out(out), {n: int(getattr(st, n)) for n, _ in HuffTrainStats._fields_}


class RateStats(C.Structure):
    """thip_enc_rate_stats (include/theoraenc_hip.h)."""
    _fields_ = [("qi", C.c_int32), ("dropped", C.c_int32), ("key", C.c_int32), ("duplicate", C.c_int32), ("target", C.c_int64),
                ("fullness_before", C.c_int64), ("fullness_after", C.c_int64), ("spend", C.c_int64), ("estimate", C.c_int64),
                ("actual", C.c_int64), ("probe", C.c_int64 * 64), ("corr", C.c_int64 * 2), ("probe_ms", C.c_double),
                ("control_ms", C.c_double)]


def make_info(w, h, fmt, quality, pic=None, fps=(30, 1), kfgshift=6, aspect=(1, 1), colorspace=0, bitrate=0):
    """A th_info for frame w x h (multiples of 16); pic = (x, y, width, height) with y from the top, default the whole frame."""
    L = _lib.load()
    info = ThInfo()
    L.th_info_init(C.byref(info))
    x, y, pw, ph = pic if pic is not None else (0, 0, w, h)
    info.frame_width, info.frame_height = w, h
    info.pic_x, info.pic_y, info.pic_width, info.pic_height = x, y, pw, ph
    info.fps_numerator, info.fps_denominator = fps
    info.aspect_numerator, info.aspect_denominator = aspect
    info.colorspace, info.pixel_fmt = colorspace, fmt
    info.target_bitrate, info.quality, info.keyframe_granule_shift = bitrate, quality, kfgshift
    return info


def _copy_packet(op):
    return C.string_at(op.packet, op.bytes) if op.bytes else b""


class Encoder:
    """th_encode_alloc -> th_encode_flushheader x3 -> {th_encode_ycbcr_in, th_encode_packetout}*."""

    def __init__(self, w, h, fmt, quality, pic=None, fps=(30, 1), kfgshift=6, device=None, comments=(), inter=False,
                 keyframe_interval=None, bitrate=None, rate_flags=None, rate_buffer=None, all_modes=False,
                 block_qi=0, device_pack=None, auto_keyframes=None, masking=0, rd_modes=False, rd_skip=False,
                 rd_quant=0, huffman=None, quant=None):
        """inter: motion-compensated inter frames (TH_ENCCTL_THIP_SET_INTER_FRAMES); keyframe_interval: then
        TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE (clamped to [1, 1 << kfgshift]; the value in force is self.keyframe_interval).
        bitrate: bits a second, bitrate mode (TH_ENCCTL_SET_BITRATE after th_encode_alloc); then rate_flags (TH_RATECTL_*) and
        rate_buffer (frames, clamped to [12, 256]; the value in force is self.rate_buffer).  all_modes: inter frames with all eight
        macro-block modes, golden-frame prediction and four vectors a macro block among them (TH_ENCCTL_THIP_SET_INTER_MODES; needs
        inter=True).  block_qi: block-level qi with that delta, 1..31 (TH_ENCCTL_THIP_SET_BLOCK_QI; 0 off).  device_pack: the device
        packetiser on (True) or off (False) through TH_ENCCTL_THIP_SET_DEVICE_PACK -- the packets are the same either way; None (the
        default) leaves the context as option "enc_device_pack" made it, which is off unless THIP_ENC_DEVICE_PACK says otherwise.
        auto_keyframes: a key frame wherever prediction stops paying, the interval becoming a maximum
        (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES): True for the recommended ratio AUTO_KEYFRAMES_DEFAULT, or the ratio t itself, 1..4096;
        None, False or 0 leave it off.  No effect without inter=True.  masking: activity masking with that ratio, 2..16
        (TH_ENCCTL_THIP_SET_MASKING; 0 off; recommended 4).  No effect without block_qi.  rd_modes: the macro-block modes of
        eight-mode inter frames by the least D + lambda R (TH_ENCCTL_THIP_SET_RD_MODES).  No effect without all_modes.  rd_skip: coded
        blocks of inter frames are left uncoded where that costs less (TH_ENCCTL_THIP_SET_RD_SKIP).  No effect without inter.
        rd_quant: the AC levels of coded blocks by the least D + lambda R with lambda's weight rd_quant / 16, 1..64
        (TH_ENCCTL_THIP_SET_RD_QUANT; 0 off; True for the recommended RD_QUANT_DEFAULT).  huffman: an (80, 32, 2) array of
        (pattern, nbits), the Huffman codes of the stream in place of the built-in ones (TH_ENCCTL_SET_HUFFMAN_CODES;
        train_huffman makes them).  quant: a QuantInfo, the quantisation parameters of the stream in place of the built-in ones
        (TH_ENCCTL_SET_QUANT_PARAMS; quant_from_headers reads another stream's)."""
        L = self._L = _lib.load()
        self.info = make_info(w, h, fmt, quality, pic, fps, kfgshift)
        self._enc = (L.th_encode_alloc(C.byref(self.info)) if device is None
                     else L.th_encode_alloc_on(C.byref(self.info), int(device)))
        if not self._enc:
            raise TheoraHipError("th_encode_alloc failed")
        self.comments = list(comments)
        if huffman is not None:
            self.set_huffman_codes(huffman)
        if quant is not None:
            self.set_quant_params(quant)
        self.hdec, self.vdec = int(not (fmt & 1)), int(not (fmt & 2))
        self.inter = bool(inter)
        self.keyframe_interval = None
        if self.inter:
            rc, _ = self.ctl(TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)
            if rc < 0:
                raise TheoraHipError("TH_ENCCTL_THIP_SET_INTER_FRAMES returned %d" % rc)
            rc, self.keyframe_interval = self.ctl(TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE,
                                                  1 << kfgshift if keyframe_interval is None else keyframe_interval, C.c_uint32)
            if rc < 0:
                raise TheoraHipError("TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE returned %d" % rc)
        elif keyframe_interval is not None:
            raise ValueError("keyframe_interval needs inter=True (an intra-only stream is all key frames)")
        self.all_modes = bool(all_modes)
        if self.all_modes:
            if not self.inter:
                raise ValueError("all_modes needs inter=True (an intra-only stream has no inter modes)")
            rc, _ = self.ctl(TH_ENCCTL_THIP_SET_INTER_MODES, 1)
            if rc < 0:
                raise TheoraHipError("TH_ENCCTL_THIP_SET_INTER_MODES returned %d" % rc)
        self.block_qi = int(block_qi)
        if self.block_qi:
            rc, _ = self.ctl(TH_ENCCTL_THIP_SET_BLOCK_QI, self.block_qi)
            if rc < 0:
                raise ValueError("block_qi must be 0..31 (TH_ENCCTL_THIP_SET_BLOCK_QI returned %d)" % rc)
        self.masking = 0
        if masking:
            self.set_masking(masking)
        self.rd_modes = False
        if rd_modes:
            self.set_rd_modes(rd_modes)
        self.rd_skip = False
        if rd_skip:
            self.set_rd_skip(rd_skip)
        self.rd_quant = 0
        if rd_quant:
            self.set_rd_quant(RD_QUANT_DEFAULT if rd_quant is True else rd_quant)
        if device_pack is not None:
            self.set_device_pack(device_pack)
        self.auto_keyframes = AUTO_KEYFRAMES_DEFAULT if auto_keyframes is True else int(auto_keyframes or 0)
        if self.auto_keyframes:
            rc, _ = self.ctl(TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, self.auto_keyframes)
            if rc < 0:
                raise ValueError("auto_keyframes must be True or 1..4096 (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES returned %d)" % rc)
        self.rate_buffer = self.bitrate = None
        if bitrate is not None:
            self.set_bitrate(bitrate)
            if rate_flags is not None:
                rc, _ = self.ctl(TH_ENCCTL_SET_RATE_FLAGS, rate_flags)
                if rc < 0:
                    raise TheoraHipError("TH_ENCCTL_SET_RATE_FLAGS returned %d" % rc)
            if rate_buffer is not None:
                rc, self.rate_buffer = self.ctl(TH_ENCCTL_SET_RATE_BUFFER, rate_buffer)
                if rc < 0:
                    raise TheoraHipError("TH_ENCCTL_SET_RATE_BUFFER returned %d" % rc)
        elif rate_flags is not None or rate_buffer is not None:
            raise ValueError("rate_flags and rate_buffer need a bitrate")

    def set_bitrate(self, bitrate):
        """TH_ENCCTL_SET_BITRATE (a long): enters bitrate mode, or changes its target from the next frame on."""
        rc, _ = self.ctl(TH_ENCCTL_SET_BITRATE, bitrate, C.c_long)
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_SET_BITRATE returned %d" % rc)
        self.bitrate = bitrate

    def set_huffman_codes(self, codes):
        """TH_ENCCTL_SET_HUFFMAN_CODES, before header_packets(): an (80, 32, 2) array of (pattern, nbits), or None for the built-in
        codes.  ValueError for codes that are no full prefix code of all 32 tokens, or too late."""
        if codes is None:
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_SET_HUFFMAN_CODES, None, 0)
        else:
            buf = _huff_codes_in(codes)
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_SET_HUFFMAN_CODES, C.byref(buf), C.sizeof(buf))
        if rc < 0:
            raise ValueError("TH_ENCCTL_SET_HUFFMAN_CODES returned %d: every set must be a full prefix-free code of all 32 tokens, "
                             "set before the first header packet" % rc)

    def set_quant_params(self, quant):
        """TH_ENCCTL_SET_QUANT_PARAMS, before header_packets(): a QuantInfo, or None for the built-in parameters.  ValueError for
        a set that is not valid, or too late."""
        if quant is None:
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_SET_QUANT_PARAMS, None, 0)
        else:
            s = quant.struct()
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_SET_QUANT_PARAMS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise ValueError("TH_ENCCTL_SET_QUANT_PARAMS returned %d: every (qti, pli) needs 1..63 ranges of sizes >= 1 summing to "
                             "63, every loop-filter limit is at most 127, set before the first header packet" % rc)

    def quant_params(self):
        """TH_ENCCTL_THIP_GET_QUANT_PARAMS: the quantisation parameters in force -> QuantInfo (a copy)."""
        s = QuantInfoStruct()
        _lib.check(self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_QUANT_PARAMS, C.byref(s), C.sizeof(s)),
                   "TH_ENCCTL_THIP_GET_QUANT_PARAMS")
        return QuantInfo.from_struct(s)

    def huffman_codes(self):
        """TH_ENCCTL_THIP_GET_HUFFMAN_CODES: the codes in force, an (80, 32, 2) array of (pattern, nbits)."""
        buf = HuffCodes()
        _lib.check(self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_HUFFMAN_CODES, C.byref(buf), C.sizeof(buf)),
                   "TH_ENCCTL_THIP_GET_HUFFMAN_CODES")
        return _huff_codes_out(buf)

    def token_hist(self):
        """TH_ENCCTL_THIP_GET_TOKEN_HIST: the last packet's merged tokens -> dict(count (5, 2, 32): Huffman group, luma / chroma,
        token; huff; key; device).  train_huffman takes a list of these."""
        h = TokenHist()
        _lib.check(self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_TOKEN_HIST, C.byref(h), C.sizeof(h)),
                   "TH_ENCCTL_THIP_GET_TOKEN_HIST")
        return _token_hist_dict(h)

    def set_masking(self, k):
        """TH_ENCCTL_THIP_SET_MASKING, before the first frame: activity masking with ratio k, 2..16 (0: off)."""
        rc, _ = self.ctl(TH_ENCCTL_THIP_SET_MASKING, int(k))
        if rc < 0:
            raise ValueError("masking must be 0 or 2..16, set before the first frame (TH_ENCCTL_THIP_SET_MASKING returned %d)" % rc)
        self.masking = int(k)

    def set_roi(self, map, stream=None):
        """TH_ENCCTL_THIP_SET_ROI_MAP: the importance map of every frame queued from now on, until the next call (include/theoraenc_hip.h,
        "Region of interest"); not between encode() and packetout().  map: a 2-D int8 numpy array or torch CUDA tensor on the
        encoder's device, entries -64..64 in 1/16 octave of lambda, positive more important, row 0 the picture's top row, of any size
        up to 16384 x 16384 (it is stretched over the picture); or a 2-D float array or tensor in octaves, read as
        clamp(round(16 x), -64, 64); or None: no map.  A tensor is read ordered on `stream` (default torch's current stream) and may
        be overwritten from that stream at once; rows may have a pitch of their own, the innermost stride must be 1.  No effect
        without block_qi."""
        a = RoiMap()
        if map is None:
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_SET_ROI_MAP, C.byref(a), C.sizeof(a))
            if rc < 0:
                raise TheoraHipError("TH_ENCCTL_THIP_SET_ROI_MAP returned %d" % rc)
            return
        host = isinstance(map, np.ndarray)
        if host:
            if map.ndim != 2:
                raise ValueError("a region-of-interest map is 2-D")
            if map.dtype.kind == "f":
                map = np.clip(np.rint(16.0 * map.astype(np.float64)), -64, 64).astype(np.int8)
            elif map.dtype != np.int8:
                raise TypeError("a region-of-interest map is int8 (1/16 octave) or float (octaves)")
            if map.strides[1] != 1:
                map = np.ascontiguousarray(map)
            shape, pitch, ptr = map.shape, map.strides[0], map.ctypes.data
        else:
            import torch
            if not isinstance(map, torch.Tensor) or not map.is_cuda:
                raise TypeError("a region-of-interest map is a numpy array or a torch CUDA tensor")
            if map.dim() != 2:
                raise ValueError("a region-of-interest map is 2-D")
            s = stream if stream is not None else torch.cuda.current_stream(map.device)
            with torch.cuda.stream(s):
                if map.dtype.is_floating_point:
                    map = torch.clamp(torch.round(16.0 * map.to(torch.float64)), -64, 64).to(torch.int8)
                elif map.dtype != torch.int8:
                    raise TypeError("a region-of-interest map is int8 (1/16 octave) or float (octaves)")
                if map.stride(1) != 1:
                    map = map.contiguous()
            shape, pitch, ptr = tuple(map.shape), map.stride(0), map.data_ptr()
            a.stream = s.cuda_stream
        if shape[0] == 0 or shape[1] == 0:
            raise ValueError("a region-of-interest map has at least one entry")
        a.height, a.width, a.device, a.pitch, a.map = shape[0], shape[1], int(not host), pitch if shape[0] > 1 else max(pitch, shape[1]), ptr
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_SET_ROI_MAP, C.byref(a), C.sizeof(a))
        if rc < 0:
            raise ValueError("the map is 1..16384 a side with entries in -64..64, set with no frame pending "
                             "(TH_ENCCTL_THIP_SET_ROI_MAP returned %d)" % rc)

    def roi_stats(self):
        """TH_ENCCTL_THIP_GET_ROI_STATS of the last packet, as a dict (without reserved)."""
        s = RoiStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_ROI_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_ROI_STATS returned %d" % rc)
        return {k: getattr(s, k) for k, _ in RoiStats._fields_ if k != "reserved"}

    def set_rd_modes(self, on):
        """TH_ENCCTL_THIP_SET_RD_MODES, before the first frame: the rate-distortion mode decision on (True) or off."""
        rc, _ = self.ctl(TH_ENCCTL_THIP_SET_RD_MODES, int(bool(on)))
        if rc < 0:
            raise ValueError("rd_modes is set before the first frame (TH_ENCCTL_THIP_SET_RD_MODES returned %d)" % rc)
        self.rd_modes = bool(on)

    def rd_stats(self):
        """TH_ENCCTL_THIP_GET_RD_STATS of the last packet, as a dict (lam: the struct's lambda)."""
        s = RdStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_RD_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_RD_STATS returned %d" % rc)
        d = {k: getattr(s, k) for k, _ in RdStats._fields_}
        d["huff"] = list(s.huff)
        return d

    def set_rd_skip(self, on):
        """TH_ENCCTL_THIP_SET_RD_SKIP, before the first frame: the skip decision on (True) or off."""
        rc, _ = self.ctl(TH_ENCCTL_THIP_SET_RD_SKIP, int(bool(on)))
        if rc < 0:
            raise ValueError("rd_skip is set before the first frame (TH_ENCCTL_THIP_SET_RD_SKIP returned %d)" % rc)
        self.rd_skip = bool(on)

    def skip_stats(self):
        """TH_ENCCTL_THIP_GET_SKIP_STATS of the last packet, as a dict (lam: the struct's lambda)."""
        s = SkipStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_SKIP_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_SKIP_STATS returned %d" % rc)
        d = {k: getattr(s, k) for k, _ in SkipStats._fields_}
        d["skipped"] = list(s.skipped)
        return d

    def set_rd_quant(self, w):
        """TH_ENCCTL_THIP_SET_RD_QUANT, before the first frame: the level choice with weight w (1..64), or off (0)."""
        rc, _ = self.ctl(TH_ENCCTL_THIP_SET_RD_QUANT, int(w))
        if rc < 0:
            raise ValueError("rd_quant is 0..64, set before the first frame (TH_ENCCTL_THIP_SET_RD_QUANT returned %d)" % rc)
        self.rd_quant = int(w)

    def rd_quant_stats(self):
        """TH_ENCCTL_THIP_GET_RD_QUANT_STATS of the last packet, as a dict (lam: the struct's lambda; without reserved)."""
        s = RdQuantStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_RD_QUANT_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_RD_QUANT_STATS returned %d" % rc)
        d = {k: getattr(s, k) for k, _ in RdQuantStats._fields_ if k != "reserved"}
        d["zeroed"], d["lowered"] = list(s.zeroed), list(s.lowered)
        return d

    def set_device_pack(self, on):
        """TH_ENCCTL_THIP_SET_DEVICE_PACK: from the next frame on (not between encode() and packetout())."""
        rc, _ = self.ctl(TH_ENCCTL_THIP_SET_DEVICE_PACK, int(bool(on)))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_SET_DEVICE_PACK returned %d" % rc)

    def pack_stats(self):
        """TH_ENCCTL_THIP_GET_PACK_STATS of the last packet, as a dict."""
        s = PackStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_PACK_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_PACK_STATS returned %d" % rc)
        return dict(device=s.device, phase=s.phase, header_bits=s.header_bits, token_bits=s.token_bits, pack_ms=s.pack_ms,
                    fallbacks=s.fallbacks)

    def ctl(self, req, value=None, ctype=C.c_int):
        v = ctype(0 if value is None else value)
        rc = self._L.th_encode_ctl(self._enc, req, C.byref(v), C.sizeof(v))
        return rc, v.value

    def header_packets(self):
        """The three header packets (bytes), with this library's vendor string and self.comments."""
        tc = ThComment()
        self._L.th_comment_init(C.byref(tc))
        for c in self.comments:
            self._L.th_comment_add(C.byref(tc), c.encode() if isinstance(c, str) else c)
        out, op = [], OggPacket()
        try:
            while True:
                rc = self._L.th_encode_flushheader(self._enc, C.byref(tc), C.byref(op))
                if rc < 0:
                    raise TheoraHipError("th_encode_flushheader returned %d" % rc)
                if rc == 0:
                    return out
                out.append(_copy_packet(op))
        finally:
            self._L.th_comment_clear(C.byref(tc))

    def encode(self, planes, stream=None):
        """Queues one frame.  planes: three uint8 numpy arrays, or three uint8 torch CUDA tensors on the encoder's device (read
        through TH_ENCCTL_THIP_YCBCR_IN_DEVICE, ordered on `stream`, default torch's current stream); each of the frame's size
        or of the picture's, rows top first."""
        if not isinstance(planes[0], np.ndarray):
            return self._encode_device(planes, stream)
        buf = (ThImgPlane * 3)()
        keep = []
        for p in range(3):
            a = np.ascontiguousarray(planes[p], dtype=np.uint8)
            keep.append(a)
            buf[p].width, buf[p].height, buf[p].stride = a.shape[1], a.shape[0], a.strides[0]
            buf[p].data = a.ctypes.data_as(C.POINTER(C.c_ubyte))
        rc = self._L.th_encode_ycbcr_in(self._enc, buf)
        if rc < 0:
            raise TheoraHipError("th_encode_ycbcr_in returned %d" % rc)

    def _encode_device(self, planes, stream):
        import torch
        a = DeviceIn()
        for p in range(3):
            t = planes[p]
            assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1
            a.planes[p].width, a.planes[p].height, a.planes[p].stride = t.shape[1], t.shape[0], t.stride(0)
            a.planes[p].data = C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_ubyte))
        s = stream if stream is not None else torch.cuda.current_stream(planes[0].device)
        a.stream = s.cuda_stream
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_YCBCR_IN_DEVICE, C.byref(a), C.sizeof(a))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_YCBCR_IN_DEVICE returned %d" % rc)

    def encode_rgb(self, image, fmt="rgb", stream=None):
        """Queues one frame given as R'G'B' (TH_ENCCTL_THIP_RGB_IN): the picture, pic_width x pic_height, as (H, W, 3) for "rgb",
        (H, W, 4) for "rgba", (3, H, W) or three (H, W) planes for "rgb_planar"; uint8 numpy arrays (host memory) or uint8 torch
        CUDA tensors on the encoder's device (ordered on `stream`, default torch's current stream; the tensor may be overwritten
        from that stream at once).  Rows may have a pitch of their own; the innermost stride must be 1."""
        if fmt not in RGB_FORMATS:
            raise ValueError("unknown R'G'B' format %r" % (fmt,))
        planes = list(image) if isinstance(image, (list, tuple)) else ([image[0], image[1], image[2]] if fmt == "rgb_planar" else [image])
        host = isinstance(planes[0], np.ndarray)
        a = RgbIn()
        a.format, a.device = RGB_FORMATS[fmt], int(not host)
        ndim, comps = (2, 1) if fmt == "rgb_planar" else (3, 4 if fmt == "rgba" else 3)
        if len(planes) != (3 if fmt == "rgb_planar" else 1):
            raise ValueError("rgb_planar wants three planes")
        for p, t in enumerate(planes):
            if host:
                if not isinstance(t, np.ndarray) or t.dtype != np.uint8:
                    raise TypeError("an R'G'B' picture is uint8 numpy arrays or uint8 torch CUDA tensors")
                strides, ptr = t.strides, t.ctypes.data
            else:
                import torch
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
                    raise TypeError("an R'G'B' picture is uint8 numpy arrays or uint8 torch CUDA tensors")
                strides, ptr = t.stride(), t.data_ptr()
            shape = tuple(t.shape)
            if len(shape) != ndim or (ndim == 3 and shape[2] != comps) or shape[:2] != tuple(planes[0].shape[:2]):
                raise ValueError("a picture of shape %s for format %r" % (shape, fmt))
            if strides[-1] != 1 or (ndim == 3 and strides[1] != comps) or strides[0] < shape[1] * comps:
                raise ValueError("R'G'B' pictures need contiguous pixels and rows (a row pitch of their own is fine)")
            a.src[p], a.pitch[p] = ptr, strides[0]
        a.height, a.width = planes[0].shape[0], planes[0].shape[1]
        if not host:
            import torch
            s = stream if stream is not None else torch.cuda.current_stream(planes[0].device)
            a.stream = s.cuda_stream
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_RGB_IN, C.byref(a), C.sizeof(a))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_RGB_IN returned %d" % rc)

    def packetout(self, last=False):
        """The next packet as (bytes, granulepos, packetno, e_o_s), or None when there is none."""
        op = OggPacket()
        rc = self._L.th_encode_packetout(self._enc, int(bool(last)), C.byref(op))
        if rc < 0:
            raise TheoraHipError("th_encode_packetout returned %d" % rc)
        if rc == 0:
            return None
        return _copy_packet(op), int(op.granulepos), int(op.packetno), int(op.e_o_s)

    def stats(self):
        """TH_ENCCTL_THIP_GET_FRAME_STATS of the last packet, as a dict."""
        s = FrameStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_FRAME_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_FRAME_STATS returned %d" % rc)
        return dict(tokens=s.tokens, tokens_merged=s.tokens_merged, bytes=s.bytes, huff=list(s.huff), overflow=s.overflow,
                    qi=s.qi)

    def times(self):
        """TH_ENCCTL_THIP_GET_TIMES: (device stage ms, host packing ms) of the last frame packet."""
        t = (C.c_double * 2)()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_TIMES, t, C.sizeof(t))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_TIMES returned %d" % rc)
        return t[0], t[1]

    def inter_stats(self):
        """TH_ENCCTL_THIP_GET_INTER_STATS of the last packet, as a dict (modes: macro blocks per mode name)."""
        s = InterStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_INTER_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_INTER_STATS returned %d" % rc)
        return dict(key=bool(s.key), modes=dict(zip(MODE_NAMES, list(s.modes))), coded=list(s.coded), mode_scheme=s.mode_scheme,
                    mv_scheme=s.mv_scheme)

    def mode_stats(self):
        """TH_ENCCTL_THIP_GET_MODE_STATS of the last packet, as a dict (modes: macro blocks per name of ALL_MODE_NAMES; vectors)."""
        s = ModeStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_MODE_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_MODE_STATS returned %d" % rc)
        return dict(modes=dict(zip(ALL_MODE_NAMES, list(s.modes))), vectors=s.vectors)

    def block_qi_stats(self):
        """TH_ENCCTL_THIP_GET_BLOCK_QI_STATS of the last packet, as a dict (blocks: coded blocks [qii][plane])."""
        s = BlockQiStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_BLOCK_QI_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_BLOCK_QI_STATS returned %d" % rc)
        return dict(nqis=s.nqis, qis=list(s.qis), blocks=[list(r) for r in s.blocks], flag_bits=s.flag_bits)

    def cut_stats(self):
        """TH_ENCCTL_THIP_GET_CUT_STATS of the last packet, as a dict."""
        s = CutStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_CUT_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_CUT_STATS returned %d" % rc)
        return {k: getattr(s, k) for k, _ in CutStats._fields_}

    def mask_stats(self):
        """TH_ENCCTL_THIP_GET_MASK_STATS of the last packet, as a dict."""
        s = MaskStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_MASK_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_MASK_STATS returned %d" % rc)
        return {k: getattr(s, k) for k, _ in MaskStats._fields_}

    def set_quality_stats(self, metrics=("sse",)):
        """TH_ENCCTL_THIP_SET_QUALITY_STATS, before the first frame: metrics "sse", ("sse", "ssim"), the THIP_CMP_* flags, or
        None / 0 for off."""
        from . import _cmp_flags
        flags = 0 if not metrics else _cmp_flags(metrics)
        rc, _ = self.ctl(TH_ENCCTL_THIP_SET_QUALITY_STATS, flags)
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_SET_QUALITY_STATS returned %d" % rc)

    def quality_stats(self):
        """TH_ENCCTL_THIP_GET_QUALITY_STATS of the last packet, as a dict: measured, flags, compare_ms and theora_amd.metrics_dict's
        keys (sse, samples, psnr, ssim, ...) over th_info's picture region.  Waits for the device."""
        from . import metrics_dict
        s = QualityStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_QUALITY_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_QUALITY_STATS returned %d" % rc)
        d = metrics_dict(list(s.sse) + list(s.samples) + list(s.ssim_q20) + list(s.windows))
        d.update(measured=s.measured, flags=s.flags, compare_ms=s.compare_ms)
        return d

    def recon(self):
        """TH_ENCCTL_THIP_GET_RECON: the encoder's reconstruction of the last frame (the next one's reference) as three uint8 numpy
        planes of the frame's size, rows top first."""
        w, h = self.info.frame_width, self.info.frame_height
        shapes = [(h, w)] + [(h >> self.vdec, w >> self.hdec)] * 2
        out = [np.empty(sh, np.uint8) for sh in shapes]
        buf = (ThImgPlane * 3)()
        for p in range(3):
            buf[p].width, buf[p].height, buf[p].stride = out[p].shape[1], out[p].shape[0], out[p].strides[0]
            buf[p].data = out[p].ctypes.data_as(C.POINTER(C.c_ubyte))
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_RECON, buf, C.sizeof(buf))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_RECON returned %d" % rc)
        return out

    def rate_stats(self):
        """TH_ENCCTL_THIP_GET_RATE_STATS of the last packet, as a dict (probe: E[0..63], corr: [c_key, c_inter])."""
        s = RateStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_RATE_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_RATE_STATS returned %d" % rc)
        d = {k: getattr(s, k) for k, _ in RateStats._fields_}
        d["probe"], d["corr"] = list(s.probe), list(s.corr)
        return d

    def two_pass_out(self):
        """TH_ENCCTL_THIP_2PASS_OUT: the next bytes of the pass file (include/theoraenc_hip.h, "Two-pass").  The first call, before
        the first frame, enters pass 1 and returns the header's placeholder; after each packetout() one call returns the packet's
        record and a second b""; after the last packet's record the next call returns the finished header, to be written over the
        placeholder at offset 0."""
        p = C.POINTER(C.c_ubyte)()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_2PASS_OUT, C.byref(p), C.sizeof(p))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_2PASS_OUT returned %d" % rc)
        return C.string_at(p, rc) if rc else b""

    def two_pass_in(self, data):
        """TH_ENCCTL_THIP_2PASS_IN: feeds bytes of the pass file, in any chunking and ahead of time; returns the bytes consumed.
        data=None asks how many more bytes the encoder wants before it can take the next frame.  The first call, before the first
        frame and in bitrate mode, enters pass 2."""
        if data is None:
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_2PASS_IN, None, 0)
        else:
            data = bytes(data)
            buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data or b"\0")
            rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_2PASS_IN, buf, len(data))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_2PASS_IN returned %d" % rc)
        return rc

    def two_pass_stats(self):
        """TH_ENCCTL_THIP_GET_2PASS_STATS of the last packet, as a dict (the struct's `pass` under "pass"; corr: [c_key, c_inter,
        and the fresh-to-recorded ratios of the two classes at the chosen qi, Q16])."""
        s = TwoPassStats()
        rc = self._L.th_encode_ctl(self._enc, TH_ENCCTL_THIP_GET_2PASS_STATS, C.byref(s), C.sizeof(s))
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_2PASS_STATS returned %d" % rc)
        d = {k: getattr(s, k) for k, _ in TwoPassStats._fields_ if k not in ("pass_", "reserved")}
        d["pass"] = s.pass_
        d["recorded"], d["fresh"], d["corr"] = list(s.recorded), list(s.fresh), list(s.corr)
        return d

    def device(self):
        rc, v = self.ctl(TH_ENCCTL_THIP_GET_DEVICE)
        if rc < 0:
            raise TheoraHipError("TH_ENCCTL_THIP_GET_DEVICE returned %d" % rc)
        return v

    def close(self):
        if getattr(self, "_enc", None):
            self._L.th_encode_free(self._enc)
            self._enc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_tokens(words_ptr, list_len, codes, lens, groups, phase, packet_ptr, cap_bytes):
    """thip_enc_pack_tokens (include/theora_hip.h): the device packetiser on the caller's tokens and tables, a test and diagnostic
    entry.  words_ptr, packet_ptr: device addresses (a tensor's data_ptr(); None is NULL); list_len [64][3], codes [80][32] and lens
    [80][32]: anything numpy converts (None is NULL).  Returns (the entry's return code, dict of thip_enc_pack_result); nothing
    is raised, the refusals are the caller's to look at."""
    L = _lib.load()
    keep = [None if a is None else np.ascontiguousarray(a, t).reshape(-1) for a, t in
            ((list_len, np.uint32), (codes, np.uint32), (lens, np.uint8))]
    for a, n in zip(keep, (192, 80 * 32, 80 * 32)):
        if a is not None and a.size != n:
            raise ValueError("pack_tokens: an array of %d entries where %d are expected" % (a.size, n))
    res = _lib.EncPackResult()
    rc = L.thip_enc_pack_tokens(words_ptr, *[None if a is None else a.ctypes.data for a in keep], int(groups), int(phase), packet_ptr,
                                int(cap_bytes), C.byref(res))
    return rc, dict(bits=res.bits, bytes=res.bytes, tokens=res.tokens, merged=res.merged, merged_ac=res.merged_ac, huff=list(res.huff))


def _stage_req(cls, frame, pixel_fmt, pic=False, planes=None, pitches=None):
    """A direct entry's request with its common part filled: frame (width, height), the pixel format, the picture where the request
    has one (pic: (x, y, width, height), None for the whole frame, False for a request without), and the groups of three it has, by
    field name: planes (device addresses, None where there is none) and pitches (None is 0)."""
    q = cls()
    q.frame_width, q.frame_height, q.pixel_fmt = int(frame[0]), int(frame[1]), int(pixel_fmt)
    if pic is not False:
        q.pic_x, q.pic_y, q.pic_width, q.pic_height = (0, 0, q.frame_width, q.frame_height) if pic is None else [int(v) for v in pic]
    for group, null, conv in ((planes or {}, None, lambda v: v), (pitches or {}, 0, int)):
        for name, v in group.items():
            for p in range(3):
                getattr(q, name)[p] = null if v is None else conv(v[p])
    return q


def _host_tables(q, who, tables):
    """Sets the request's host tables: (field, value, dtype, entries) each, the value anything numpy converts; None stays NULL, and
    entries None takes any size.  who: what a ValueError for a wrong size begins with.  Returns the arrays, to be kept alive over
    the call."""
    keep = []
    for name, v, t, size in tables:
        if v is None:
            continue
        a = np.ascontiguousarray(v, t).reshape(-1)
        if size is not None and a.size != size:
            raise ValueError("%s %s of %d entries where %d are expected" % (who, name, a.size, size))
        keep.append(a)
        setattr(q, name, a.ctypes.data)
    return keep


def _qi_tables(nqis, dequant, bits):
    """skip_stage's and rdq_stage's tables: dequant [nqis][2][3][64] -- of any size with an nqis the entry refuses: the refusal is its
    to make -- and bits [2][4][32]."""
    return [("dequant", dequant, np.uint16, 384 * int(nqis) if 1 <= int(nqis) <= 3 else None), ("bits", bits, np.uint8, 256)]


def tok_stage(frame, pixel_fmt, classes, stages, levels=None, dcq=None, dcr=None, cmap=None, tok=None, mask=None, chunk_cnt=None,
              chunk_base=None, list_len=None, overflow=None, out=None, out_cap=0):
    """thip_enc_tok_stage (include/theora_hip.h): the tokeniser on the caller's levels, DCs and map, a test and diagnostic entry.
    frame: (width, height); classes: 0 (a key frame), 2 or 3; stages: an OR of _lib.ENC_TOK_*; out_cap: the words of out; the rest:
    device addresses (a tensor's data_ptr(); None is NULL).  Returns the entry's return code; nothing is raised, the refusals are the
    caller's to look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncTokReq, frame, pixel_fmt)
    q.classes, q.stages, q.out_cap = int(classes), int(stages), int(out_cap)
    q.levels, q.dcq, q.dcr, q.cmap, q.tok, q.mask = levels, dcq, dcr, cmap, tok, mask
    q.chunk_cnt, q.chunk_base, q.list_len, q.overflow, q.out = chunk_cnt, chunk_base, list_len, overflow, out
    return L.thip_enc_tok_stage(C.byref(q))


def inter_stage(frame, pixel_fmt, stages, classes, pic=None, lam=0, src=None, src_pitch=None, prev=None, gold=None, ref_pitch=None,
                dequant=None, stats=None, words=None, words_from_stats=None, levels=None, dcq=None, cmap=None, dcr=None):
    """thip_enc_inter_stage (include/theora_hip.h): the device stage of an inter frame on the caller's planes, lambda and tables, a
    test and diagnostic entry.  frame: (width, height); pic: (x, y, width, height), the whole frame when None; stages: an OR of
    _lib.ENC_INTER_*; src, prev, gold: three device addresses each (a tensor's data_ptr(); None where there is none) with their
    pitches; dequant [2][3][64]: anything numpy converts; the rest: device addresses, None is NULL.  Returns the entry's return
    code; nothing is raised, the refusals are the caller's to look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncInterReq, frame, pixel_fmt, pic, dict(src=src, prev=prev, gold=gold), dict(src_pitch=src_pitch, ref_pitch=ref_pitch))
    q.stages, q.lam, q.classes = int(stages), int(lam), int(classes)
    keep = _host_tables(q, "inter_stage: a", [("dequant", dequant, np.uint16, 384)])
    q.stats, q.words, q.words_from_stats, q.levels, q.dcq, q.cmap, q.dcr = stats, words, words_from_stats, levels, dcq, cmap, dcr
    return L.thip_enc_inter_stage(C.byref(q))


def rate_stage(frame, pixel_fmt, inter, stages, pic=None, groups=0, fixed=0, src=None, src_pitch=None, prev=None, ref_pitch=None,
               steps=None, lam=None, lens=None, stats=None, coef=None, qdc=None, coded=None, cls=None, partial=None, est=None,
               any_order=0):
    """thip_enc_rate_stage (include/theora_hip.h): the rate probe's stages on the caller's buffers and tables, a test and diagnostic
    entry.  frame: (width, height); pic: (x, y, width, height), the whole frame when None; stages: an OR of _lib.ENC_RATE_*; src,
    prev: three device addresses each (None where there is none) with their pitches; steps [6][64][64], lam [64] and lens [80][32]:
    anything numpy converts (None is NULL); the rest: device addresses, None is NULL.  any_order: 1 lets the steps rise and fall
    with q in any way (thip_enc_rate_req.any_order).  Returns the entry's return code; nothing is raised, the refusals are the
    caller's to look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncRateReq, frame, pixel_fmt, pic, dict(src=src, prev=prev), dict(src_pitch=src_pitch, ref_pitch=ref_pitch))
    q.inter, q.stages, q.groups, q.fixed, q.any_order = int(inter), int(stages), int(groups), int(fixed), int(any_order)
    keep = _host_tables(q, "rate_stage:", [("steps", steps, np.uint16, 6 * 64 * 64), ("lam", lam, np.int32, 64), ("lens", lens, np.uint8, 80 * 32)])
    q.stats, q.coef, q.qdc, q.coded, q.cls, q.partial, q.est = stats, coef, qdc, coded, cls, partial, est
    return L.thip_enc_rate_stage(C.byref(q))


def mask_stage(frame, pixel_fmt, ratio, pic=None, src=None, src_pitch=None, act=None, avg=None, iscale=None):
    """thip_enc_mask_stage (include/theora_hip.h): the activity map and the scales of activity masking on the caller's planes, a test
    and diagnostic entry.  frame: (width, height); pic: (x, y, width, height), the whole frame when None; ratio: k; src: three
    device addresses (None where there is none) with their pitches; act (uint32 [nluma]), avg (uint64 [2]) and iscale (uint16
    [nfrags]): device addresses, None is NULL.  Returns the entry's return code; nothing is raised, the refusals are the caller's to
    look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncMaskReq, frame, pixel_fmt, pic, dict(src=src), dict(src_pitch=src_pitch))
    q.ratio = int(ratio)
    q.act, q.avg, q.iscale = act, avg, iscale
    return L.thip_enc_mask_stage(C.byref(q))


def roi_stage(frame, pixel_fmt, map_size, map_pitch, map, pic=None, mask_iscale=None, iscale=None, stats=None):
    """thip_enc_roi_stage (include/theora_hip.h): the scales of a region-of-interest map, a test and diagnostic entry.  frame: (width,
    height); pic: (x, y, width, height), the whole frame when None; map_size: (width, height) of the map; map (int8 rows at
    map_pitch), mask_iscale (uint16 [nfrags], masking's scales), iscale (uint16 [nfrags]) and stats (int32 [8]): device addresses,
    None is NULL.  Returns the entry's return code; nothing is raised, the refusals are the caller's to look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncRoiReq, frame, pixel_fmt, pic)
    q.map_width, q.map_height, q.map_pitch = int(map_size[0]), int(map_size[1]), int(map_pitch)
    q.map, q.mask_iscale, q.iscale, q.stats = map, mask_iscale, iscale, stats
    return L.thip_enc_roi_stage(C.byref(q))


def rd_stage(frame, pixel_fmt, stages, pic=None, lambda_search=0, lambda_rd=0, src=None, src_pitch=None, prev=None, gold=None,
             ref_pitch=None, dequant=None, bits=None, cand=None, costs=None, words=None):
    """thip_enc_rd_stage (include/theora_hip.h): the rate-distortion mode decision on the caller's planes, lambdas and tables, a test
    and diagnostic entry.  frame: (width, height); pic: (x, y, width, height), the whole frame when None; stages: an OR of
    _lib.ENC_RD_*; src, prev, gold: three device addresses each (None where there is none) with their pitches; dequant [2][3][64]
    and bits [2][5][32]: anything numpy converts (None is NULL); cand, costs, words: device addresses, None is NULL.  Returns the
    entry's return code; nothing is raised, the refusals are the caller's to look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncRdReq, frame, pixel_fmt, pic, dict(src=src, prev=prev, gold=gold), dict(src_pitch=src_pitch, ref_pitch=ref_pitch))
    q.stages, q.lambda_search, q.lambda_rd = int(stages), int(lambda_search), int(lambda_rd)
    keep = _host_tables(q, "rd_stage:", [("dequant", dequant, np.uint16, 384), ("bits", bits, np.uint8, 320)])
    q.cand, q.costs, q.words = cand, costs, words
    return L.thip_enc_rd_stage(C.byref(q))


def skip_stage(frame, pixel_fmt, classes, nqis, pic=None, lam=-1, src=None, src_pitch=None, prev=None, gold=None, ref_pitch=None,
               words=None, dequant=None, bits=None, iscale=None, levels=None, dcq=None, qii=None, cmap=None, skf=None, dcode=None,
               rate=None, dskip=None):
    """thip_enc_skip_stage (include/theora_hip.h): the skip decision on the caller's planes, words and tables, a test and diagnostic
    entry.  frame: (width, height); pic: (x, y, width, height), the whole frame when None; classes: 2 (32-bit words) or 3 (16-byte
    words, gold given); lam: the unscaled lambda of every block, -1 for each block's own; src, prev, gold: three device addresses each
    (None where there is none) with their pitches; dequant [nqis][2][3][64] and bits [2][4][32]: anything numpy converts (None is
    NULL); the rest: device addresses, None is NULL.  Returns the entry's return code; nothing is raised, the refusals are the
    caller's to look at."""
    L = _lib.load()
    q = _stage_req(_lib.EncSkipReq, frame, pixel_fmt, pic, dict(src=src, prev=prev, gold=gold), dict(src_pitch=src_pitch, ref_pitch=ref_pitch))
    q.classes, q.nqis, q.lam = int(classes), int(nqis), int(lam)
    keep = _host_tables(q, "skip_stage:", _qi_tables(nqis, dequant, bits))
    q.words, q.iscale, q.levels, q.dcq, q.qii, q.cmap, q.skf = words, iscale, levels, dcq, qii, cmap, skf
    q.dcode, q.rate, q.dskip = dcode, rate, dskip
    return L.thip_enc_skip_stage(C.byref(q))


def fq_stage(frame, pixel_fmt, classes, nqis, pic=None, src=None, src_pitch=None, prev=None, gold=None, ref_pitch=None, words=None,
             dequant=None, bits=None, iscale=None, levels=None, dcq=None, qii=None, cmap=None, dcr=None, overflow=None):
    """thip_enc_fq_stage (include/theora_hip.h): the transform-and-quantise kernels on the caller's planes, words and tables, a test
    and diagnostic entry.  classes: 0 (a key frame: prev, gold, words, cmap, dcr unused), 2 or 3; nqis: 0 (the plain kernel: bits,
    qii unused) or 1..3 (the block-qi kernel, with iscale the masked one); dequant [max(nqis, 1)][2][3][64], with classes 0
    [max(nqis, 1)][3][64]; the rest as skip_stage takes them.  Returns the entry's return code; nothing is raised."""
    L = _lib.load()
    q = _stage_req(_lib.EncFqReq, frame, pixel_fmt, pic, dict(src=src, prev=prev, gold=gold), dict(src_pitch=src_pitch, ref_pitch=ref_pitch))
    q.classes, q.nqis = int(classes), int(nqis)
    # (of any size with an nqis or classes the entry refuses: the refusal is its to make)
    size = max(int(nqis), 1) * (192 if int(classes) == 0 else 384) if 0 <= int(nqis) <= 3 and int(classes) in (0, 2, 3) else None
    keep = _host_tables(q, "fq_stage:", [("dequant", dequant, np.uint16, size), ("bits", bits, np.uint8, 256)])
    q.words, q.iscale, q.levels, q.dcq, q.qii, q.cmap, q.dcr, q.overflow = words, iscale, levels, dcq, qii, cmap, dcr, overflow
    return L.thip_enc_fq_stage(C.byref(q))


def rdq_stage(frame, pixel_fmt, classes, nqis, weight, pic=None, lam=-1, src=None, src_pitch=None, prev=None, gold=None,
              ref_pitch=None, words=None, dequant=None, bits=None, iscale=None, levels=None, qii=None, cmap=None, jbefore=None,
              jafter=None, rate=None):
    """thip_enc_rdq_stage (include/theora_hip.h): the level choice on the caller's planes, words, tables and levels, a test and
    diagnostic entry.  classes: 0 (a key frame: prev, gold, words, cmap unused), 2 or 3; weight: w; levels: device address, in and
    out; the rest as skip_stage takes them.  Returns the entry's return code; nothing is raised."""
    L = _lib.load()
    q = _stage_req(_lib.EncRdqReq, frame, pixel_fmt, pic, dict(src=src, prev=prev, gold=gold), dict(src_pitch=src_pitch, ref_pitch=ref_pitch))
    q.classes, q.nqis, q.weight, q.lam = int(classes), int(nqis), int(weight), int(lam)
    keep = _host_tables(q, "rdq_stage:", _qi_tables(nqis, dequant, bits))
    q.words, q.iscale, q.levels, q.qii, q.cmap = words, iscale, levels, qii, cmap
    q.jbefore, q.jafter, q.rate = jbefore, jafter, rate
    return L.thip_enc_rdq_stage(C.byref(q))


def rate_groups(nfrags):
    """thip_enc_rate_groups (include/theora_hip.h): the work groups the probe's token stage takes for nfrags blocks (host code)."""
    return _lib.load().thip_enc_rate_groups(int(nfrags))


def ogg_stream(header_packets, data_packets, serialno=0x7E0):
    """One Ogg logical stream (bytes) through the library's writer (include/thip_ogg.h): the headers, a flush after the setup
    header, then data_packets as (payload, granulepos, e_o_s)."""
    L = _lib.load()
    w = L.thip_ogg_writer_new(serialno)
    if not w:
        raise TheoraHipError("thip_ogg_writer_new failed")
    out = []
    try:
        allp = [(p, 0, 0) for p in header_packets] + list(data_packets)
        for k, (payload, gp, eos) in enumerate(allp):
            buf = (C.c_ubyte * max(len(payload), 1)).from_buffer_copy(bytes(payload) if payload else b"\0")
            op = OggPacket(C.cast(buf, C.c_void_p), len(payload), int(k == 0), int(eos), gp, k)
            if L.thip_ogg_writer_packetin(w, C.byref(op)) != 0:
                raise TheoraHipError("thip_ogg_writer_packetin(packet %d) failed" % k)
            if k == len(header_packets) - 1:
                L.thip_ogg_writer_flush(w)
            n = C.c_size_t()
            p = L.thip_ogg_writer_pages(w, C.byref(n))
            out.append(C.string_at(p, n.value) if n.value else b"")
        L.thip_ogg_writer_flush(w)
        n = C.c_size_t()
        p = L.thip_ogg_writer_pages(w, C.byref(n))
        out.append(C.string_at(p, n.value) if n.value else b"")
    finally:
        L.thip_ogg_writer_free(w)
    return b"".join(out)
