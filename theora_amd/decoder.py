"""Python face of the th_decode_* API exported by libtheora_hip.so (include/theoradec_hip.h):
the calls a libtheoradec user makes, in the order they make them."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OggPacket, ThComment, ThImgPlane, ThInfo, TheoraHipError

TH_DUPFRAME = 1
TH_DECCTL_GET_PPLEVEL_MAX, TH_DECCTL_SET_PPLEVEL, TH_DECCTL_SET_GRANPOS, TH_DECCTL_SET_STRIPE_CB = 1, 3, 5, 7
TH_DECCTL_THIP_GET_SLOT_TRACE = 0x7101
TH_DECCTL_THIP_SET_DEVICE_DC = 0x7102
TH_DECCTL_THIP_SET_DEVICE_TOKENS = 0x7103
TH_DECCTL_THIP_SET_DEVICE_LISTS = 0x7104
TH_DECCTL_THIP_PREFETCH_PACKET = 0x7105
TH_DECCTL_THIP_GET_DEVICE = 0x7106
TH_DECCTL_THIP_SET_HOST_OUTPUT = 0x7107
TH_DECCTL_THIP_PICTURE_OUT = 0x7108


class PictureOutArgs(C.Structure):
    """thip_picture_out_args (include/theoradec_hip.h)."""
    _fields_ = [("format", C.c_int32), ("chroma", C.c_int32), ("crop", C.c_int32), ("dst", C.c_void_p * 3),
                ("dst_pitch", C.c_int64 * 3), ("stream", C.c_void_p)]


TH_DECCTL_THIP_PICTURE_RESIZE = 0x7109


class PictureResizeArgs(C.Structure):
    """thip_picture_resize_args (include/theoradec_hip.h)."""
    _fields_ = [("format", C.c_int32), ("filter", C.c_int32), ("elem", C.c_int32),
                ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("out_width", C.c_int32), ("out_height", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3),
                ("dst", C.c_void_p * 3), ("dst_pitch", C.c_int64 * 3), ("stream", C.c_void_p)]


TH_DECCTL_THIP_PICTURE_COMPARE = 0x710A


class PictureCompareArgs(C.Structure):
    """thip_picture_compare_args (include/theoradec_hip.h)."""
    _fields_ = [("flags", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("ref", C.c_void_p * 3), ("ref_pitch", C.c_int64 * 3), ("result", C.c_void_p),
                ("block_sse", C.c_void_p * 3), ("block_pitch", C.c_int64 * 3), ("stream", C.c_void_p)]


TH_DECCTL_THIP_SET_FRAME_INFO = 0x710B
TH_DECCTL_THIP_FRAME_INFO_OUT = 0x710C


class FrameInfoArgs(C.Structure):
    """thip_frame_info_args (include/theoradec_hip.h)."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("crop", C.c_int32),
                ("elem", C.c_int32), ("refs", C.c_int32), ("reserved", C.c_int32),
                ("kind", C.c_void_p * 3), ("kind_pitch", C.c_int64 * 3), ("mv", C.c_void_p * 3), ("mv_pitch", C.c_int64 * 3),
                ("ncoef", C.c_void_p * 3), ("ncoef_pitch", C.c_int64 * 3), ("flow", C.c_void_p), ("flow_pitch", C.c_int64),
                ("valid", C.c_void_p), ("valid_pitch", C.c_int64), ("stream", C.c_void_p),
                ("frame_type", C.c_int32), ("nqis", C.c_int32), ("qis", C.c_int32 * 3), ("ncoded", C.c_int32)]


STRIPE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(ThImgPlane), C.c_int, C.c_int)


class StripeCallback(C.Structure):
    """th_stripe_callback (theoradec.h:79-92)."""
    _fields_ = [("ctx", C.c_void_p), ("stripe_decoded", STRIPE_FN)]


class SlotTrace(C.Structure):
    """thip_slot_trace (include/theoradec_hip.h)."""
    _fields_ = [("ncoded", C.c_int64), ("fragi", C.POINTER(C.c_int32)), ("pli", C.POINTER(C.c_uint8)),
                ("last_zzi", C.POINTER(C.c_uint8)), ("refi", C.POINTER(C.c_uint8)),
                ("dc_quant", C.POINTER(C.c_uint16)), ("mv", C.POINTER(C.c_int16)),
                ("coeffs", C.POINTER(C.c_int16)), ("nuncoded", C.c_int64), ("uncoded", C.POINTER(C.c_int64)),
                ("flimit", C.c_int32), ("frame_type", C.c_int32)]


def _packet(data, bos=0, packetno=0):
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(bytes(data) if len(data) else b"\0")
    op = OggPacket(C.cast(buf, C.c_void_p), len(data), bos, 0, -1, packetno)
    return op, buf


class Decoder:
    """th_decode_headerin x3 -> th_decode_alloc -> {th_decode_packetin, th_decode_ycbcr_out}*."""

    def __init__(self, header_packets, device=None):
        L = self._L = _lib.load()
        self.info = ThInfo()
        self.comment = ThComment()
        L.th_info_init(C.byref(self.info))
        L.th_comment_init(C.byref(self.comment))
        setup = C.c_void_p()
        for k, pkt in enumerate(header_packets):
            op, keep = _packet(pkt, bos=1 if k == 0 else 0, packetno=k)
            rc = L.th_decode_headerin(C.byref(self.info), C.byref(self.comment), C.byref(setup), C.byref(op))
            if rc <= 0:
                raise TheoraHipError("th_decode_headerin(packet %d) returned %d" % (k, rc))
        self._dec = (L.th_decode_alloc(C.byref(self.info), setup) if device is None
                     else L.th_decode_alloc_on(C.byref(self.info), setup, int(device)))
        L.th_setup_free(setup)
        if not self._dec:
            raise TheoraHipError("th_decode_alloc failed")
        self._npackets = len(header_packets)

    def packetin_raw(self, data):
        """th_decode_packetin as it is: (rc, granulepos), a negative rc included; nothing is raised."""
        op, keep = _packet(data, packetno=self._npackets)
        self._npackets += 1
        gp = C.c_int64(-1)
        rc = self._L.th_decode_packetin(self._dec, C.byref(op), C.byref(gp))
        return rc, gp.value

    def packetin(self, data):
        """Returns (rc, granulepos); rc 0 = new frame, TH_DUPFRAME = repeat of the last one."""
        rc, gp = self.packetin_raw(data)
        if rc < 0:
            raise TheoraHipError("th_decode_packetin returned %d" % rc)
        return rc, gp

    def ctl(self, req, buf, size):
        """th_decode_ctl as it is: buf a ctypes object (or None), size in bytes; the return code, nothing is raised."""
        return self._L.th_decode_ctl(self._dec, int(req), None if buf is None else C.byref(buf), int(size))

    def set_granpos(self, granpos, size=None):
        """TH_DECCTL_SET_GRANPOS (a seek: the next frame counts on from here); the return code.  size: buf_sz, if not the value's."""
        v = C.c_int64(granpos)
        return self.ctl(TH_DECCTL_SET_GRANPOS, v, C.sizeof(v) if size is None else size)

    def set_pp_level(self, level):
        """TH_DECCTL_SET_PPLEVEL, 0 .. 7; the return code."""
        v = C.c_int(level)
        return self.ctl(TH_DECCTL_SET_PPLEVEL, v, C.sizeof(v))

    def pp_level_max(self):
        """TH_DECCTL_GET_PPLEVEL_MAX: (return code, value)."""
        v = C.c_int(-1)
        rc = self.ctl(TH_DECCTL_GET_PPLEVEL_MAX, v, C.sizeof(v))
        return rc, v.value

    def set_stripe_cb(self, fn, ctx=None):
        """TH_DECCTL_SET_STRIPE_CB: fn(ctx, th_ycbcr_buffer, first fragment row, end fragment row) is called from inside
        packetin() for every decoded frame; None switches it off.  The return code."""
        cb = STRIPE_FN(fn) if fn is not None else STRIPE_FN()
        s = StripeCallback(ctx, cb)
        rc = self.ctl(TH_DECCTL_SET_STRIPE_CB, s, C.sizeof(s))
        if rc == 0:
            self._stripe_keep = cb          # (the library calls it until it is replaced)
        return rc

    def prefetch(self, data):
        """TH_DECCTL_THIP_PREFETCH_PACKET: announce a packet that a later packetin() will bring (decode order).  True when
        it was taken; the pictures are the same either way."""
        op, keep = _packet(data)
        rc = self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_PREFETCH_PACKET, C.byref(op), C.sizeof(op))
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_PREFETCH_PACKET returned %d" % rc)
        return rc == 0

    def ycbcr_out(self):
        """Three numpy planes, display order (top row first), the full coded frame."""
        buf = (ThImgPlane * 3)()
        rc = self._L.th_decode_ycbcr_out(self._dec, buf)
        if rc < 0:
            raise TheoraHipError("th_decode_ycbcr_out returned %d" % rc)
        out = []
        for p in buf:
            a = np.ctypeslib.as_array(p.data, (p.height, p.stride))[:, :p.width]
            out.append(a.copy())
        return out

    def device(self):
        """TH_DECCTL_THIP_GET_DEVICE: the GPU the context decodes on."""
        v = C.c_int(-1)
        rc = self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_GET_DEVICE, C.byref(v), C.sizeof(v))
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_GET_DEVICE returned %d" % rc)
        return v.value

    def set_host_output(self, on):
        """TH_DECCTL_THIP_SET_HOST_OUTPUT: False stops the copy of every decoded frame to the host image (ycbcr_out() then copies
        on demand)."""
        v = C.c_int(int(bool(on)))
        rc = self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_SET_HOST_OUTPUT, C.byref(v), C.sizeof(v))
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_SET_HOST_OUTPUT returned %d" % rc)

    def picture(self, fmt="rgb", chroma="linear", crop=True, stream=None, out=None):
        """TH_DECCTL_THIP_PICTURE_OUT: the picture of the frame packetin() last returned as a uint8 device tensor ((H, W, 3),
        (H, W, 4), (3, H, W), or three planes for "ycbcr"); crop: th_info's picture region, else the whole coded frame.
        Asynchronous on `stream` (default: torch's current stream).  `out`: destination(s) of those shapes to write instead."""
        import torch
        from . import CHROMA_MODES, PIC_FORMATS, _on_stream, _pic_dst, picture_shapes
        i = self.info
        x, y, w, h = (i.pic_x, i.pic_y, i.pic_width, i.pic_height) if crop else (0, 0, i.frame_width, i.frame_height)
        shapes = picture_shapes(fmt, w, h, x, i.pixel_fmt, y)
        dev = self.device()
        if out is None:
            td = torch.device("cuda", dev)
            out = (tuple(torch.empty(s, dtype=torch.uint8, device=td) for s in shapes) if fmt == "ycbcr"
                   else torch.empty(shapes, dtype=torch.uint8, device=td))
        ptrs, pitches = _pic_dst(fmt, out, shapes)
        a = PictureOutArgs()
        a.format, a.chroma, a.crop = PIC_FORMATS[fmt], CHROMA_MODES[chroma], int(bool(crop))
        for p in range(3):
            a.dst[p] = ptrs[p]
            a.dst_pitch[p] = pitches[p]

        def call(hs):
            a.stream = hs
            return self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_PICTURE_OUT, C.byref(a), C.sizeof(a))
        rc = _on_stream(dev, stream, call)
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_PICTURE_OUT returned %d" % rc)
        return out

    def picture_resized(self, size, fmt="rgb_planar", filter="area", rect=None, dtype=None, scale=None, bias=None, stream=None,
                        out=None):
        """TH_DECCTL_THIP_PICTURE_RESIZE: the rectangle `rect` = (x, y, width, height) of the frame packetin() last returned (None:
        the whole coded frame) resampled to size = (out_width, out_height), as a device tensor of theora_amd.picture_resize_shapes'
        shapes: uint8, or for "rgb_planar" torch.float16 / torch.float32 holding c * scale[k] + bias[k].  Asynchronous on `stream`
        (default: torch's current stream).  `out`: destination(s) of those shapes to write instead."""
        import torch
        from . import FILTERS, PIC_FORMATS, _elem, _on_stream, _pic_dst, picture_resize_shapes
        dtype = torch.uint8 if dtype is None else dtype
        shapes = picture_resize_shapes(fmt, size[0], size[1], self.info.pixel_fmt)
        dev = self.device()
        if out is None:
            td = torch.device("cuda", dev)
            out = (tuple(torch.empty(s, dtype=dtype, device=td) for s in shapes) if fmt == "ycbcr"
                   else torch.empty(shapes, dtype=dtype, device=td))
        ptrs, pitches = _pic_dst(fmt, out, shapes, dtype)
        a = PictureResizeArgs()
        a.format, a.filter, a.elem = PIC_FORMATS[fmt], FILTERS[filter], _elem(dtype)
        a.x, a.y, a.width, a.height = rect if rect is not None else (0, 0, 0, 0)
        a.out_width, a.out_height = size
        for p in range(3):
            a.scale[p] = 1.0 if scale is None else scale[p]
            a.bias[p] = 0.0 if bias is None else bias[p]
            a.dst[p] = ptrs[p]
            a.dst_pitch[p] = pitches[p]

        def call(hs):
            a.stream = hs
            return self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_PICTURE_RESIZE, C.byref(a), C.sizeof(a))
        rc = _on_stream(dev, stream, call)
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_PICTURE_RESIZE returned %d" % rc)
        return out

    def picture_compare(self, ref, metrics=("sse",), rect=None, stream=None, result=None):
        """TH_DECCTL_THIP_PICTURE_COMPARE: the rectangle `rect` = (x, y, width, height) of the frame packetin() last returned (None:
        the whole coded frame) against `ref`, three uint8 device planes of theora_amd.picture_shapes("ycbcr", ...)'s shapes.  Returns
        the (12,) int64 device tensor of thip_picture_metrics (theora_amd.metrics_dict reads it); `result`: such a tensor to write
        instead.  Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        from . import _cmp_flags, _on_stream, picture_shapes
        dev = self.device()
        if result is None:
            result = torch.empty(12, dtype=torch.int64, device=torch.device("cuda", dev))
        a = PictureCompareArgs()
        a.flags = _cmp_flags(metrics)
        a.x, a.y, a.width, a.height = rect if rect is not None else (0, 0, 0, 0)
        x, y, w, h = rect if rect is not None else (0, 0, self.info.frame_width, self.info.frame_height)
        shapes = picture_shapes("ycbcr", w, h, x, self.info.pixel_fmt, y)      # (the library reads exactly these planes)
        for p in range(3):
            t = ref[p]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
                raise TypeError("reference pictures are 2-D uint8 device tensors")
            if tuple(t.shape) != tuple(shapes[p]) or t.stride(0) < t.shape[1]:
                raise ValueError("reference plane %d of shape %s for a plane of %s" % (p, tuple(t.shape), tuple(shapes[p])))
            a.ref[p], a.ref_pitch[p] = t.data_ptr(), t.stride(0)
        if result.dtype != torch.int64 or result.numel() != 12 or not result.is_cuda or not result.is_contiguous():
            raise TypeError("a result is a contiguous int64 device tensor of 12 elements")
        a.result = result.data_ptr()

        def call(hs):
            a.stream = hs
            return self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_PICTURE_COMPARE, C.byref(a), C.sizeof(a))
        rc = _on_stream(dev, stream, call)
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_PICTURE_COMPARE returned %d" % rc)
        return result

    def set_frame_info(self, on):
        """TH_DECCTL_THIP_SET_FRAME_INFO: True keeps a record of every frame's side data from the next packet on, for
        frame_info(); the return code."""
        v = C.c_int(int(bool(on)))
        return self.ctl(TH_DECCTL_THIP_SET_FRAME_INFO, v, C.sizeof(v))

    def frame_info(self, what=("kind", "mv", "flow"), rect=None, dtype=None, refs=("prev",), crop=True, stream=None, out=None):
        """TH_DECCTL_THIP_FRAME_INFO_OUT: the side data of the frame packetin() last returned (set_frame_info(True) before it) as
        a dict of new device tensors of theora_amd.frame_info_shapes' shapes -- any of "kind", "mv", "ncoef" (three planes each),
        "flow" (dtype torch.float16, the default, or torch.float32; refs: "prev", "gold" or both) and "valid" -- plus the host
        fields "frame_type", "nqis", "qis" and "ncoded".  crop: th_info's picture region, else `rect` = (x, y, width, height),
        None: the whole coded frame.  Asynchronous on `stream`.  `out`: a dict of destinations to write instead."""
        import torch
        from . import _elem, _fi_refs, _on_stream, frame_info_alloc, frame_info_shapes
        i = self.info
        x, y, w, h = (i.pic_x, i.pic_y, i.pic_width, i.pic_height) if crop else \
            (rect if rect is not None else (0, 0, i.frame_width, i.frame_height))
        dev = self.device()
        if out is None:
            out = frame_info_alloc(frame_info_shapes(w, h, x, y, i.pixel_fmt), what, torch.float16 if dtype is None else dtype,
                                   torch.device("cuda", dev))
        a = FrameInfoArgs()
        a.crop = int(bool(crop))
        if not crop and rect is not None:
            a.x, a.y, a.width, a.height = rect
        a.refs = _fi_refs(refs)
        for key in ("kind", "mv", "ncoef"):
            for p, t in enumerate(out.get(key) or ()):
                if t is not None:
                    getattr(a, key)[p] = t.data_ptr()
                    getattr(a, key + "_pitch")[p] = t.stride(0)
        if out.get("flow") is not None:
            t = out["flow"]
            a.flow, a.flow_pitch, a.elem = t.data_ptr(), t.stride(1) * t.element_size(), _elem(t.dtype)
        if out.get("valid") is not None:
            a.valid, a.valid_pitch = out["valid"].data_ptr(), out["valid"].stride(0)

        def call(hs):
            a.stream = hs
            return self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_FRAME_INFO_OUT, C.byref(a), C.sizeof(a))
        rc = _on_stream(dev, stream, call)
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_FRAME_INFO_OUT returned %d" % rc)
        res = dict(out)
        res.update(frame_type=int(a.frame_type), nqis=int(a.nqis), qis=[int(q) for q in a.qis][:int(a.nqis)], ncoded=int(a.ncoded))
        return res

    def slot_trace(self):
        """The accel-vtable slot calls of the last frame as numpy arrays; only on a context
        allocated with THIP_FE_TRACE_BACKEND=1 in the environment (no device needed)."""
        t = SlotTrace()
        rc = self._L.th_decode_ctl(self._dec, TH_DECCTL_THIP_GET_SLOT_TRACE, C.byref(t), C.sizeof(t))
        if rc < 0:
            raise TheoraHipError("TH_DECCTL_THIP_GET_SLOT_TRACE returned %d" % rc)
        n, u = int(t.ncoded), int(t.nuncoded)

        def arr(ptr, count, shape=None):
            if count == 0:
                return np.zeros(shape or (0,), np.ctypeslib.as_array(ptr, (1,)).dtype if ptr else np.int64)
            a = np.ctypeslib.as_array(ptr, (count,)).copy()
            return a.reshape(shape) if shape else a

        return dict(fragi=arr(t.fragi, n), pli=arr(t.pli, n), last_zzi=arr(t.last_zzi, n), refi=arr(t.refi, n),
                    dc_quant=arr(t.dc_quant, n), mv=arr(t.mv, n), coeffs=arr(t.coeffs, n * 64, (n, 64)),
                    uncoded=arr(t.uncoded, u), flimit=int(t.flimit), frame_type=int(t.frame_type))

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


def ogg_packets(data):
    """Packets of a physical Ogg bitstream held in `data` (bytes), in page order, through the
    library's demultiplexer (include/thip_ogg.h): a list of (serialno, payload, b_o_s, e_o_s,
    granulepos, packetno) and the (bad_pages, gaps) counters."""
    L = _lib.load()
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(bytes(data) if len(data) else b"\0")
    r = L.thip_ogg_open_memory(C.cast(buf, C.c_void_p), len(data))
    if not r:
        raise TheoraHipError("thip_ogg_open_memory failed")
    out = []
    op, serial = OggPacket(), C.c_uint32()
    while L.thip_ogg_next_packet(r, C.byref(op), C.byref(serial)) == 1:
        payload = C.string_at(op.packet, op.bytes) if op.bytes else b""
        out.append((serial.value, payload, int(op.b_o_s), int(op.e_o_s), int(op.granulepos), int(op.packetno)))
    bad, gaps = C.c_int64(), C.c_int64()
    L.thip_ogg_stats(r, C.byref(bad), C.byref(gaps))
    L.thip_ogg_close(r)
    return out, (bad.value, gaps.value)
