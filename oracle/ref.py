"""The reference codec itself, built from its own source tree into oracle/_ref/libtheora_ref.so and driven through ctypes --
TEST INFRASTRUCTURE ONLY, like the rest of this package.

The recipe: the pure-C translation units named below, straight from the reference tree (nothing of it is copied into this
repository), with oracle/ref_shim/ standing in for libogg (types and a bit writer, written here).  oracle/_ref/ is a build
product: git ignores it, a machine that has the reference tree makes it, a machine that has not uses the one that came with the
working tree or goes without.

libtheora_hip.so exports th_decode_* / th_encode_* under the same names.  Both libraries live in one process without binding into
each other: each is dlopen()ed RTLD_LOCAL, and this one is linked -Bsymbolic so that its own calls stay inside it
(tests/test_reference_cpu.py::test_two_libraries_one_process)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
SO = os.path.join(REF_DIR, "libtheora_ref.so")
SHIM = os.path.join(_HERE, "ref_shim")
# where the reference's source tree is; a machine without it does not build
TREE = os.environ.get("THEORA_REFERENCE_TREE", "/root/reference")

# lib/*.c of the reference: the decoder's and the encoder's lists, C only (no OC_X86_ASM)
DEC_UNITS = ("apiwrapper", "bitpack", "decapiwrapper", "decinfo", "decode", "dequant", "fragment", "huffdec", "idct", "info",
             "internal", "quant", "state")
ENC_UNITS = ("analyze", "encapiwrapper", "encfrag", "encinfo", "encode", "enquant", "fdct", "huffenc", "mathops", "mcenc", "rate",
             "tokenize")

TH_EFAULT, TH_EINVAL, TH_EBADHEADER, TH_ENOTFORMAT, TH_EVERSION, TH_EIMPL, TH_EBADPACKET, TH_DUPFRAME = -1, -10, -20, -21, -22, -23, -24, 1
TH_DECCTL_GET_PPLEVEL_MAX, TH_DECCTL_SET_PPLEVEL, TH_DECCTL_SET_GRANPOS = 1, 3, 5
TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE, TH_ENCCTL_SET_SPLEVEL, TH_ENCCTL_SET_RATE_FLAGS, TH_ENCCTL_SET_RATE_BUFFER = 4, 14, 20, 22
TH_ENCCTL_SET_QUALITY, TH_ENCCTL_SET_BITRATE = 28, 30


def tree_present():
    return os.path.isfile(os.path.join(TREE, "lib", "decode.c"))


def available():
    """True when the library exists or can be built here."""
    return os.path.exists(SO) or tree_present()


def build(force=False, quiet=False):
    """Compile the reference into oracle/_ref/libtheora_ref.so; returns its path, or None where there is neither the tree nor a
    library.  Without the tree nothing is done and an existing oracle/_ref/ is left alone.  Portable flags only: the library is
    made on one machine and loaded on another."""
    def say(msg):
        if not quiet:
            print("oracle.ref: " + msg, file=sys.stderr)
    if not tree_present():
        if os.path.exists(SO):
            say("no reference tree at %s; using the existing %s" % (TREE, os.path.relpath(SO, os.path.dirname(_HERE))))
            return SO
        say("no reference tree at %s and no oracle/_ref/: the reference-pinned tests will skip" % TREE)
        return None
    own = [os.path.join(SHIM, "ogg", "ogg.h"), os.path.join(SHIM, "bitwriter.c"), os.path.abspath(__file__)]
    if not force and os.path.exists(SO) and os.path.getmtime(SO) >= max(os.path.getmtime(p) for p in own):
        return SO
    os.makedirs(REF_DIR, exist_ok=True)
    srcs = [os.path.join(TREE, "lib", u + ".c") for u in DEC_UNITS + ENC_UNITS] + [os.path.join(SHIM, "bitwriter.c")]
    tmp = SO + ".tmp%d" % os.getpid()
    cmd = [os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", "-w", "-Wl,-Bsymbolic", "-I" + SHIM,
           "-I" + os.path.join(TREE, "include"), "-I" + os.path.join(TREE, "lib")] + srcs + ["-o", tmp, "-lm"]
    try:
        subprocess.check_call(cmd)
        os.replace(tmp, SO)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    say("built %s from %s" % (os.path.relpath(SO, os.path.dirname(_HERE)), TREE))
    return SO


class ThInfo(C.Structure):
    """th_info (theora/codec.h)."""
    _fields_ = [("version_major", C.c_ubyte), ("version_minor", C.c_ubyte), ("version_subminor", C.c_ubyte),
                ("frame_width", C.c_uint32), ("frame_height", C.c_uint32), ("pic_width", C.c_uint32),
                ("pic_height", C.c_uint32), ("pic_x", C.c_uint32), ("pic_y", C.c_uint32),
                ("fps_numerator", C.c_uint32), ("fps_denominator", C.c_uint32),
                ("aspect_numerator", C.c_uint32), ("aspect_denominator", C.c_uint32),
                ("colorspace", C.c_int), ("pixel_fmt", C.c_int), ("target_bitrate", C.c_int),
                ("quality", C.c_int), ("keyframe_granule_shift", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ThComment(C.Structure):
    _fields_ = [("user_comments", C.POINTER(C.c_char_p)), ("comment_lengths", C.POINTER(C.c_int)),
                ("comments", C.c_int), ("vendor", C.c_char_p)]


class OggPacket(C.Structure):
    _fields_ = [("packet", C.c_void_p), ("bytes", C.c_long), ("b_o_s", C.c_long), ("e_o_s", C.c_long),
                ("granulepos", C.c_int64), ("packetno", C.c_int64)]


class ThImgPlane(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("stride", C.c_int), ("data", C.POINTER(C.c_ubyte))]


_lib = None


def lib():
    """The reference library (built on demand where the tree is); raises where it can be neither found nor built."""
    global _lib
    if _lib is not None:
        return _lib
    so = build(quiet=True)
    if so is None:
        raise RuntimeError("oracle/_ref/libtheora_ref.so is missing and there is no reference tree at %s: "
                           "__graft_entry__.build() makes it where the tree is" % TREE)
    L = C.CDLL(so, mode=getattr(os, "RTLD_LOCAL", 0) | os.RTLD_NOW)
    P, I, U, I64 = C.c_void_p, C.c_int, C.c_uint, C.c_int64
    for name, res, args in (
            ("th_info_init", None, [C.POINTER(ThInfo)]), ("th_info_clear", None, [C.POINTER(ThInfo)]),
            ("th_comment_init", None, [C.POINTER(ThComment)]), ("th_comment_clear", None, [C.POINTER(ThComment)]),
            ("th_decode_headerin", I, [C.POINTER(ThInfo), C.POINTER(ThComment), C.POINTER(P), C.POINTER(OggPacket)]),
            ("th_decode_alloc", P, [C.POINTER(ThInfo), P]), ("th_setup_free", None, [P]),
            ("th_decode_ctl", I, [P, I, P, C.c_size_t]),
            ("th_decode_packetin", I, [P, C.POINTER(OggPacket), C.POINTER(I64)]),
            ("th_decode_ycbcr_out", I, [P, C.POINTER(ThImgPlane)]), ("th_decode_free", None, [P]),
            ("th_granule_frame", I64, [P, I64]), ("th_version_string", C.c_char_p, []),
            ("th_encode_alloc", P, [C.POINTER(ThInfo)]), ("th_encode_ctl", I, [P, I, P, C.c_size_t]),
            ("th_encode_flushheader", I, [P, C.POINTER(ThComment), C.POINTER(OggPacket)]),
            ("th_encode_ycbcr_in", I, [P, C.POINTER(ThImgPlane)]),
            ("th_encode_packetout", I, [P, I, C.POINTER(OggPacket)]), ("th_encode_free", None, [P]),
            # the block kernels (state.h, encint.h: the accel vtable's C entries)
            ("oc_idct8x8_c", None, [P, P, I]), ("oc_enc_fdct8x8_c", None, [P, P]),
            ("oc_frag_copy_c", None, [P, P, I]), ("oc_frag_recon_intra_c", None, [P, I, P]),
            ("oc_frag_recon_inter_c", None, [P, P, I, P]), ("oc_frag_recon_inter2_c", None, [P, P, P, I, P]),
            ("oc_loop_filter_init_c", None, [P, I]),
            ("oc_enc_frag_sub_c", None, [P, P, P, I]), ("oc_enc_frag_sub_128_c", None, [P, P, I]),
            ("oc_enc_frag_sad_c", U, [P, P, I]), ("oc_enc_frag_sad_thresh_c", U, [P, P, I, U]),
            ("oc_enc_frag_sad2_thresh_c", U, [P, P, P, I, U]), ("oc_enc_frag_intra_sad_c", U, [P, I]),
            ("oc_enc_frag_satd_c", U, [C.POINTER(I), P, P, I]), ("oc_enc_frag_satd2_c", U, [C.POINTER(I), P, P, P, I]),
            ("oc_enc_frag_intra_satd_c", U, [C.POINTER(I), P, I]), ("oc_enc_frag_ssd_c", U, [P, P, I]),
            ("oc_enc_frag_border_ssd_c", U, [P, P, I, I64]), ("oc_enc_frag_copy2_c", None, [P, P, P, I]),
            ("oc_enc_enquant_table_init_c", None, [P, P]), ("oc_enc_quantize_c", I, [P, P, P, P])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    _lib = L
    return L


def _packet(data, bos=0, packetno=0):
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(bytes(data) if len(data) else b"\0")
    return OggPacket(C.cast(buf, C.c_void_p), len(data), bos, 0, -1, packetno), buf


def _planes_out(buf):
    out = []
    for p in buf:
        if p.stride >= p.width:
            out.append(np.ctypeslib.as_array(p.data, (p.height, p.stride))[:, :p.width].copy())
        else:       # a negative stride: row y is at data + y * stride all the same
            base = C.addressof(p.data.contents)
            out.append(np.stack([np.frombuffer(C.string_at(base + y * p.stride, p.width), np.uint8) for y in range(p.height)]))
    return out


def headerin(header_packets):
    """th_decode_headerin over the packets: (return codes, th_info, setup handle or None, comment).  The caller frees."""
    L = lib()
    info, tc, setup = ThInfo(), ThComment(), C.c_void_p()
    L.th_info_init(C.byref(info))
    L.th_comment_init(C.byref(tc))
    rcs = []
    for k, pkt in enumerate(header_packets):
        op, keep = _packet(pkt, bos=int(k == 0), packetno=k)
        rcs.append(L.th_decode_headerin(C.byref(info), C.byref(tc), C.byref(setup), C.byref(op)))
    return rcs, info, setup, tc


class RefDecoder:
    """The reference's th_decode_headerin x3 -> th_decode_alloc -> {th_decode_packetin, th_decode_ycbcr_out}*."""

    def __init__(self, header_packets):
        L = self._L = lib()
        rcs, self.info, setup, self.comment = headerin(header_packets)
        if any(rc <= 0 for rc in rcs):
            L.th_setup_free(setup)
            L.th_comment_clear(C.byref(self.comment))
            raise ValueError("reference th_decode_headerin returned %r" % rcs)
        self._dec = L.th_decode_alloc(C.byref(self.info), setup)
        L.th_setup_free(setup)
        if not self._dec:
            L.th_comment_clear(C.byref(self.comment))
            raise ValueError("reference th_decode_alloc failed")
        self._npackets = len(header_packets)

    def packetin(self, data):
        """(rc, granulepos): rc 0 = new frame, TH_DUPFRAME = repeat, negative = refused.  Nothing is raised."""
        op, keep = _packet(data, packetno=self._npackets)
        self._npackets += 1
        gp = C.c_int64(-1)
        rc = self._L.th_decode_packetin(self._dec, C.byref(op), C.byref(gp))
        return rc, gp.value

    def ctl(self, req, buf, size):
        return self._L.th_decode_ctl(self._dec, req, buf, size)

    def set_pp_level(self, n):
        v = C.c_int(n)
        rc = self.ctl(TH_DECCTL_SET_PPLEVEL, C.byref(v), C.sizeof(v))
        if rc < 0:
            raise ValueError("TH_DECCTL_SET_PPLEVEL(%d) returned %d" % (n, rc))

    def pp_level_max(self):
        v = C.c_int(-1)
        self.ctl(TH_DECCTL_GET_PPLEVEL_MAX, C.byref(v), C.sizeof(v))
        return v.value

    def granule_frame(self, gp):
        return self._L.th_granule_frame(self._dec, gp)

    def ycbcr_out(self):
        """Three numpy planes, display order (top row first), the full coded frame."""
        buf = (ThImgPlane * 3)()
        rc = self._L.th_decode_ycbcr_out(self._dec, buf)
        if rc < 0:
            raise ValueError("reference th_decode_ycbcr_out returned %d" % rc)
        return _planes_out(buf)

    def close(self):
        if getattr(self, "_dec", None):
            self._L.th_decode_free(self._dec)
            self._dec = None
            self._L.th_comment_clear(C.byref(self.comment))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RefEncoder:
    """The reference's th_encode_alloc -> th_encode_flushheader* -> {th_encode_ycbcr_in, th_encode_packetout*}*.
    pic = (x, y, width, height), y from the top as th_info has it; quality 0..63 or bitrate in bits a second."""

    def __init__(self, w, h, fmt=0, pic=None, quality=32, bitrate=0, kf_interval=64, fps=(30, 1), speed=None, rate_flags=None,
                 rate_buffer=None):
        L = self._L = lib()
        info = self.info = ThInfo()
        L.th_info_init(C.byref(info))
        x, y, pw, ph = pic if pic is not None else (0, 0, w, h)
        info.frame_width, info.frame_height = w, h
        info.pic_x, info.pic_y, info.pic_width, info.pic_height = x, y, pw, ph
        info.fps_numerator, info.fps_denominator = fps
        info.aspect_numerator = info.aspect_denominator = 1
        info.colorspace, info.pixel_fmt = 0, fmt
        info.target_bitrate, info.quality = bitrate, quality
        shift = 0
        while (1 << shift) < kf_interval:           # ilog(kf_interval - 1), as the reference's example encoder sets it
            shift += 1
        info.keyframe_granule_shift = shift
        self._enc = L.th_encode_alloc(C.byref(info))
        if not self._enc:
            raise ValueError("reference th_encode_alloc failed")
        rc, self.keyframe_interval = self.ctl(TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE, kf_interval, C.c_uint32)
        assert rc == 0, rc
        if speed is not None:
            assert self.ctl(TH_ENCCTL_SET_SPLEVEL, speed)[0] == 0
        if rate_flags is not None:
            assert self.ctl(TH_ENCCTL_SET_RATE_FLAGS, rate_flags)[0] == 0
        if rate_buffer is not None:
            assert self.ctl(TH_ENCCTL_SET_RATE_BUFFER, rate_buffer)[0] == 0
        self.hdec, self.vdec = int(not (fmt & 1)), int(not (fmt & 2))

    def ctl(self, req, value, ctype=C.c_int):
        v = ctype(value)
        rc = self._L.th_encode_ctl(self._enc, req, C.byref(v), C.sizeof(v))
        return rc, v.value

    def header_packets(self):
        tc = ThComment()
        self._L.th_comment_init(C.byref(tc))
        out, op = [], OggPacket()
        while True:
            rc = self._L.th_encode_flushheader(self._enc, C.byref(tc), C.byref(op))
            if rc < 0:
                raise ValueError("reference th_encode_flushheader returned %d" % rc)
            if rc == 0:
                return out
            out.append(C.string_at(op.packet, op.bytes))

    def encode(self, planes, last=False):
        """One frame in (three uint8 planes of the frame's size, rows top first); the packets it makes, as
        [(bytes, granulepos)] -- more than one only with duplicates."""
        buf = (ThImgPlane * 3)()
        keep = []
        for p in range(3):
            a = np.ascontiguousarray(planes[p], dtype=np.uint8)
            keep.append(a)
            buf[p].width, buf[p].height, buf[p].stride = a.shape[1], a.shape[0], a.strides[0]
            buf[p].data = a.ctypes.data_as(C.POINTER(C.c_ubyte))
        rc = self._L.th_encode_ycbcr_in(self._enc, buf)
        if rc < 0:
            raise ValueError("reference th_encode_ycbcr_in returned %d" % rc)
        out, op = [], OggPacket()
        while True:
            rc = self._L.th_encode_packetout(self._enc, int(bool(last)), C.byref(op))
            if rc < 0:
                raise ValueError("reference th_encode_packetout returned %d" % rc)
            if rc == 0:
                return out
            out.append((C.string_at(op.packet, op.bytes) if op.bytes else b"", int(op.granulepos)))

    def close(self):
        if getattr(self, "_enc", None):
            self._L.th_encode_free(self._enc)
            self._enc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the block kernels, one call a block ----------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def idct8x8(x, last_zzi):
    """oc_idct8x8_c over [n,64] int16 (natural order), last_zzi scalar or [n]; the input is not changed."""
    L = lib()
    x = np.ascontiguousarray(x, np.int16).reshape(-1, 64)
    lz = np.broadcast_to(np.asarray(last_zzi, np.int32), (x.shape[0],))
    y = np.zeros_like(x)
    tmp = np.zeros(64, np.int16)
    for i in range(x.shape[0]):
        tmp[:] = x[i]
        L.oc_idct8x8_c(_p(y[i]), _p(tmp), int(lz[i]))
    return y


def fdct8x8(x):
    """oc_enc_fdct8x8_c over [n,64] int16 residuals."""
    L = lib()
    x = np.ascontiguousarray(x, np.int16).reshape(-1, 64)
    y = np.zeros_like(x)
    for i in range(x.shape[0]):
        L.oc_enc_fdct8x8_c(_p(y[i]), _p(x[i]))
    return y


def loop_filter_bv(flimit):
    bv = np.zeros(256, np.int8)
    lib().oc_loop_filter_init_c(_p(bv), flimit)
    return bv


ENQUANT_BYTES = 64 * 4          # oc_iquant{int16 m, l}[64] (enquant.h)


def quantize(dct, dequant):
    """oc_enc_enquant_table_init_c + oc_enc_quantize_c over [n,64] coefficients with one 64-entry table: (levels, nonzero)."""
    L = lib()
    d = np.ascontiguousarray(dct, np.int16).reshape(-1, 64)
    dq = np.ascontiguousarray(dequant, np.uint16)
    enq = np.zeros(ENQUANT_BYTES + 64, np.uint8)
    L.oc_enc_enquant_table_init_c(_p(enq), _p(dq))
    q = np.zeros_like(d)
    nz = np.zeros(d.shape[0], np.int32)
    for i in range(d.shape[0]):
        nz[i] = L.oc_enc_quantize_c(_p(q[i]), _p(d[i]), _p(dq), _p(enq))
    return q, nz


def metric(op, src_plane, ref_plane, ystride, src_offs, ref_offs=None, ref2_offs=None, thresh=0):
    """The reference's own slot for every block, same arguments and ops as oracle.enc_metric_batch: (values, dc)."""
    L = lib()
    sp = np.ascontiguousarray(src_plane, np.uint8)
    rp = sp if ref_plane is None else np.ascontiguousarray(ref_plane, np.uint8)
    s0, r0 = sp.ctypes.data, rp.ctypes.data
    n = len(src_offs)
    out, dcs = np.zeros(n, np.uint32), np.zeros(n, np.int32)
    dc = C.c_int(0)
    for i in range(n):
        s = s0 + int(src_offs[i])
        r = None if ref_offs is None else r0 + int(ref_offs[i])
        r2 = None if ref2_offs is None else r0 + int(ref2_offs[i])
        dc.value = 0
        if op == "sad":
            v = L.oc_enc_frag_sad_c(s, r, ystride)
        elif op == "sad_thresh":
            v = L.oc_enc_frag_sad_thresh_c(s, r, ystride, thresh)
        elif op == "sad2_thresh":
            v = L.oc_enc_frag_sad2_thresh_c(s, r, r2, ystride, thresh)
        elif op == "intra_sad":
            v = L.oc_enc_frag_intra_sad_c(s, ystride)
        elif op == "satd":
            v = L.oc_enc_frag_satd_c(C.byref(dc), s, r, ystride)
        elif op == "satd2":
            v = L.oc_enc_frag_satd2_c(C.byref(dc), s, r, r2, ystride)
        elif op == "intra_satd":
            v = L.oc_enc_frag_intra_satd_c(C.byref(dc), s, ystride)
        elif op == "ssd":
            v = L.oc_enc_frag_ssd_c(s, r, ystride)
        else:
            raise ValueError(op)
        out[i], dcs[i] = v, dc.value
    return out, dcs
