"""theora_amd -- MI355X (gfx950) backend for libtheora's per-fragment reconstruction path.

The product is the C-ABI library ``libtheora_hip.so`` (include/theora_hip.h, sources in
theora_amd/csrc/).  This package is the thin Python harness above it used by tests and
bench.py: ctypes bindings, host-side packing of fragment command streams into the
backend's HBM layout, and device-buffer plumbing through torch.  It never falls back to a
CPU implementation.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (DUPFRAME, FRAME_GOLD, FRAME_PREV, FRAME_SELF, INTER_FRAME, INTRA_FRAME,  # noqa: F401
                   COEFFS_DEQUANT16, COEFFS_LEVELS, MAX_BATCH, SLOT_GROUP, SLOT_GROUP_BYTES, SLOT_WIDE, TILE_FRAGS, FrameDesc,
                   PlaneGeom, TheoraHipError, TileGeom)

TILE_BLOCKS = SLOT_GROUP   # slots per coefficient group

PF_420, PF_422, PF_444 = 0, 2, 3


def version():
    return _lib.load().thip_version_string().decode()


def _ptr(t):
    """Device (torch tensor) or host (numpy array) address, or NULL."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


# ---------------------------------------------------------------------------------------
# host-side packing of a frame's fragment command stream (layout of include/theora_hip.h)
# ---------------------------------------------------------------------------------------
def info_words(npos, pos, refi, last_zzi, mvx, mvy, dc, dc_quant, qii=None):
    """[npos,2] uint32 frag_info array (include/theora_hip.h): coded fragments at tile
    positions `pos`; every other position stays 0 (uncoded / outside the plane).  dc is the raw
    DC coefficient (used for the DC-only fragments, whose value has no coefficient slot),
    dc_quant the per-fragment DC quantiser: the dequantisation itself (state.c:967-979) is the
    kernel's.  qii given: the LEVELS form -- word 0 carries it, word 1 the raw DC of every block."""
    out = np.zeros((npos, 2), np.uint32)
    lz = np.asarray(last_zzi, np.uint32)
    w0 = np.uint32(_lib.INFO_CODED) | ((np.asarray(refi, np.uint32) & 3) << 1) | (lz << 8)
    w0 |= np.where(lz < 2, np.uint32(_lib.INFO_DC_ONLY), np.uint32(0))
    w0 |= (np.asarray(mvx, np.int32).astype(np.uint32) & 0xFF) << 16
    w0 |= (np.asarray(mvy, np.int32).astype(np.uint32) & 0xFF) << 24
    if qii is not None:
        w0 |= (np.asarray(qii, np.uint32) & 3) << _lib.INFO_QII_SHIFT
    out[pos, 0] = w0
    w1 = (np.asarray(dc_quant, np.int64).astype(np.uint32) & 0xFFFF) << 16
    w1 |= np.where((lz < 2) | (qii is not None), np.asarray(dc, np.int32).astype(np.uint32) & 0xFFFF, 0).astype(np.uint32)
    out[pos, 1] = w1
    return out


def pack_tiles(coeffs):
    """[n,64] natural-order int16 blocks -> the backend's tile layout (int16, flat); see
    include/theora_hip.h: group q=2j+h of slot i at group(i//64)*4096 + q*512 + (i%64)*8
    int16s, holding {x[2j][c], x[2j+1][c]} for c=4h..4h+3."""
    co = np.asarray(coeffs, np.int16).reshape(-1, 8, 8)
    n = co.shape[0]
    ntiles = (n + TILE_BLOCKS - 1) // TILE_BLOCKS
    pad = np.zeros((ntiles * TILE_BLOCKS, 8, 8), np.int16)
    pad[:n] = co
    # [tile, lane, j, half, h, cc] -> [tile, j, h, lane, cc, half]
    t = pad.reshape(ntiles, TILE_BLOCKS, 4, 2, 2, 4).transpose(0, 2, 4, 1, 5, 3)
    return np.ascontiguousarray(t).reshape(-1)


def pack_units(levels, wide, first_unit, nunits):
    """The LEVELS form's slot array (include/theora_hip.h): levels [n,64] natural-order int16, wide [n] bool (the block's
    tile is wide), first_unit [n] the block's first 64-byte unit.  Returns the array as uint8, whole groups of 64 units."""
    lv = np.asarray(levels, np.int16).reshape(-1, 8, 8)
    wide = np.asarray(wide, bool)
    first_unit = np.asarray(first_unit, np.int64)
    ngroups = (int(nunits) + 63) // 64
    out = np.zeros(ngroups * 4096, np.uint8)

    def addr(unit, piece):     # byte address of a unit's piece
        return (unit >> 6) * 4096 + piece * 1024 + (unit & 63) * 16
    nar = np.nonzero(~wide)[0]
    if nar.size:
        # piece j, dword d: bytes x[2j][2d], x[2j][2d+1], x[2j+1][2d], x[2j+1][2d+1]
        b = lv[nar].astype(np.int8).reshape(-1, 4, 2, 4, 2).transpose(0, 1, 3, 2, 4)      # [n, j, d, parity, e]
        b = np.ascontiguousarray(b).reshape(-1, 4, 16).view(np.uint8)
        for j in range(4):
            a = addr(first_unit[nar], j)
            out[(a[:, None] + np.arange(16)[None, :]).reshape(-1)] = b[:, j].reshape(-1)
    wd = np.nonzero(wide)[0]
    if wd.size:
        # piece q = 2j+h: the int16 pairs {x[2j][c], x[2j+1][c]}, c = 4h..4h+3; pieces 0-3 in the first unit, 4-7 in the second
        t = lv[wd].reshape(-1, 4, 2, 2, 4).transpose(0, 1, 3, 4, 2)                        # [n, j, h, cc, parity]
        t = np.ascontiguousarray(t).reshape(-1, 8, 8).view(np.uint8).reshape(-1, 8, 16)
        for q in range(8):
            a = addr(first_unit[wd] + (q >> 2), q & 3)
            out[(a[:, None] + np.arange(16)[None, :]).reshape(-1)] = t[:, q].reshape(-1)
    return out


def pack_dequant_tables(dequant):
    """[3][3][2][64] zig-zag-ordered uint16 tables -> the 18 x 64 slot-order array the kernels multiply with
    (what thip_pack_dequant_table does for one table): out[(j*8 + c)*2 + p] = table[zig-zag index of (2j+p, c)]."""
    from .synth import FZIG_ZAG
    dq = np.ascontiguousarray(dequant, np.uint16).reshape(18, 64)
    nat = np.zeros((18, 64), np.uint16)
    nat[:, FZIG_ZAG] = dq
    return np.ascontiguousarray(nat.reshape(18, 4, 2, 8).transpose(0, 1, 3, 2)).reshape(18, 64)


def unpack_tiles(tiles, n):
    t = np.asarray(tiles, np.int16).reshape(-1, 4, 2, TILE_BLOCKS, 4, 2).transpose(0, 3, 1, 5, 2, 4)
    return np.ascontiguousarray(t).reshape(-1, 64)[:n]


class State:
    """Device side of one stream (thip_state): three resident frames + the reference ring."""

    def __init__(self, frame_width, frame_height, pixel_fmt=PF_420, device=None):
        self._L = _lib.load()
        h = C.c_void_p()
        if device is None:      # the calling thread's current HIP device
            _lib.check(self._L.thip_state_create(C.byref(h), frame_width, frame_height, pixel_fmt),
                       "thip_state_create")
        else:
            _lib.check(self._L.thip_state_create_on(C.byref(h), int(device), frame_width, frame_height, pixel_fmt),
                       "thip_state_create_on")
        self.device = self._L.thip_state_device(h)
        self._h = h
        geom = (PlaneGeom * 3)()
        nfrags, fbytes = C.c_int64(), C.c_int64()
        _lib.check(self._L.thip_state_get_geom(h, geom, C.byref(nfrags), C.byref(fbytes)), "get_geom")
        self.planes = [dict((f, getattr(g, f)) for f, _ in PlaneGeom._fields_) for g in geom]
        self.nfrags = nfrags.value
        self.frame_bytes = fbytes.value
        self.frame_width, self.frame_height, self.pixel_fmt = frame_width, frame_height, pixel_fmt
        tg = TileGeom()
        _lib.check(self._L.thip_state_get_tiles(h, C.byref(tg)), "get_tiles")
        self.tiles_x, self.tiles_y, self.tile_off = list(tg.tiles_x), list(tg.tiles_y), list(tg.tile_off)
        self.ntiles = tg.ntiles

    def frag_pos(self, fragi):
        return self._L.thip_state_frag_pos(self._h, int(fragi))

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._L.thip_state_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ref_idx(self, which):
        return self._L.thip_state_ref_idx(self._h, which)

    def check_fault(self):
        """thip_state_check_fault: waits for the state's stream; 0 nothing wrong, 1 the newest frame was decoded again (a tile
        hand-over had failed), raises on THIP_EFAULT.  For callers that only bracket their work with synchronize()."""
        return _lib.check(self._L.thip_state_check_fault(self._h), "thip_state_check_fault")

    def set_ref_idx(self, gold, prev, self_):
        _lib.check(self._L.thip_state_set_ref_idx(self._h, gold, prev, self_), "set_ref_idx")

    def read_plane(self, bufi, pli):
        g = self.planes[pli]
        out = np.empty((g["height"], g["width"]), np.uint8)
        _lib.check(self._L.thip_state_read_plane(self._h, bufi, pli, out.ctypes.data), "read_plane")
        return out

    def write_plane(self, bufi, pli, arr):
        g = self.planes[pli]
        a = np.ascontiguousarray(arr, np.uint8)
        assert a.shape == (g["height"], g["width"])
        _lib.check(self._L.thip_state_write_plane(self._h, bufi, pli, a.ctypes.data), "write_plane")

    def ycbcr_out(self):
        """th_decode_ycbcr_out: the last decoded frame, display (top-down) row order."""
        outs = [np.empty((g["height"], g["width"]), np.uint8) for g in self.planes]
        ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
        strides = (C.c_int32 * 3)(*[g["width"] for g in self.planes])
        _lib.check(self._L.thip_state_ycbcr_out(self._h, ptrs, strides), "ycbcr_out")
        return outs

    def ycbcr_map(self):
        """The same frame without the copy: numpy views of the library's pinned image (valid
        until the second following frame has been decoded; do not write)."""
        ptrs = (C.c_void_p * 3)()
        strides = (C.c_int32 * 3)()
        _lib.check(self._L.thip_state_ycbcr_map(self._h, ptrs, strides), "ycbcr_map")
        outs = []
        for pli, g in enumerate(self.planes):
            buf = (C.c_ubyte * (strides[pli] * g["height"])).from_address(ptrs[pli])
            outs.append(np.frombuffer(buf, np.uint8).reshape(g["height"], strides[pli])[:, :g["width"]])
        return outs

    def picture(self, fmt="rgb", chroma="linear", rect=None, bufi=-1, stream=None):
        """The state's newest picture (or ring buffer `bufi` as decoded) as a new uint8 device tensor: (H, W, 3), (H, W, 4),
        (3, H, W), or a tuple of three planes for "ycbcr".  rect = (x, y, width, height) in display coordinates, None = the whole
        coded frame.  Asynchronous on `stream` (default: torch's current stream), like picture_out."""
        import torch
        x, y, w, h = rect if rect is not None else (0, 0, self.frame_width, self.frame_height)
        shapes = picture_shapes(fmt, w, h, x, self.pixel_fmt, y)
        dev = torch.device("cuda", self.device)
        if fmt == "ycbcr":
            out = tuple(torch.empty(s, dtype=torch.uint8, device=dev) for s in shapes)
        else:
            out = torch.empty(shapes, dtype=torch.uint8, device=dev)
        picture_out([self], [out], fmt, chroma, [rect], [bufi], stream)
        return out

    def picture_resized(self, size, fmt="rgb_planar", filter="area", rect=None, bufi=-1, dtype=None, scale=None, bias=None,
                        stream=None):
        """The state's newest picture (or ring buffer `bufi` as decoded), the rectangle `rect` of it (None: the whole coded frame),
        resampled to size = (out_width, out_height) as a new device tensor of picture_resize_shapes' shapes: uint8, or for
        "rgb_planar" torch.float16 / torch.float32 holding c * scale[k] + bias[k] per channel.  filter: "area" (the one for
        downscaling) or "bilinear".  Asynchronous on `stream` (default: torch's current stream), like picture_resize."""
        import torch
        dtype = torch.uint8 if dtype is None else dtype
        shapes = picture_resize_shapes(fmt, size[0], size[1], self.pixel_fmt)
        dev = torch.device("cuda", self.device)
        if fmt == "ycbcr":
            out = tuple(torch.empty(s, dtype=dtype, device=dev) for s in shapes)
        else:
            out = torch.empty(shapes, dtype=dtype, device=dev)
        picture_resize([self], [out], [size], fmt, filter, [rect], [bufi], dtype, scale, bias, stream)
        return out

    def compare(self, ref, metrics=("sse",), rect=None, bufi=-1, blocks=False, stream=None):
        """The state's newest picture (or ring buffer `bufi` as decoded), the rectangle `rect` of it (None: the whole coded frame),
        compared with `ref`, three uint8 device planes of picture_shapes("ycbcr", ...)'s shapes: picture_compare for one state,
        with result tensors made here.  Returns the (12,) int64 device tensor of thip_picture_metrics (metrics_dict reads it), or
        with blocks=True that and the three uint32-valued (int32 dtype) block_sse tensors.  Asynchronous on `stream`."""
        import torch
        dev = torch.device("cuda", self.device)
        res = torch.empty(12, dtype=torch.int64, device=dev)
        blk = None
        if blocks:
            x, y, w, h = rect if rect is not None else (0, 0, self.frame_width, self.frame_height)
            blk = [torch.empty(((sh[0] + 7) // 8, (sh[1] + 7) // 8), dtype=torch.int32, device=dev)
                   for sh in picture_shapes("ycbcr", w, h, x, self.pixel_fmt, y)]
        picture_compare([self], [ref], [res], metrics, [rect], [bufi], None if blk is None else [blk], stream)
        return (res, blk) if blocks else res

    def set_frame_info(self, on):
        """thip_state_set_frame_info: keep a record of the side data of every frame this state decodes from now on."""
        _lib.check(self._L.thip_state_set_frame_info(self._h, int(bool(on))), "set_frame_info")

    def frame_info(self, what=("kind", "mv", "flow"), rect=None, dtype=None, refs=("prev",), frag_info=None, stream=None):
        """The side data of the frame decoded last (set_frame_info must be on), or of the frame whose frag_info words `frag_info`
        holds (a device tensor, tile order), as a dict of new device tensors: frame_info for one state.  what: any of "kind",
        "mv", "ncoef" (lists of three planes), "flow" (dtype torch.float16, the default, or torch.float32) and "valid".
        Asynchronous on `stream`."""
        import torch
        x, y, w, h = rect if rect is not None else (0, 0, self.frame_width, self.frame_height)
        out = frame_info_alloc(frame_info_shapes(w, h, x, y, self.pixel_fmt), what, torch.float16 if dtype is None else dtype,
                               torch.device("cuda", self.device))
        frame_info([self], [out], [rect], refs, None if frag_info is None else [frag_info], stream)
        return out

    def set_eager_output(self, on):
        _lib.check(self._L.thip_state_set_eager_output(self._h, int(bool(on))), "set_eager_output")

    # ---- host-enqueue form: the vtable slots, one fragment at a time --------------------
    def frame_begin(self, frame_type):
        _lib.check(self._L.thip_frame_begin(self._h, frame_type), "frame_begin")

    def frag_recon(self, fragi, pli, dct_coeffs, last_zzi, dc_quant, refi, mv):
        """oc_state_frag_recon slot; dct_coeffs is an int16[128] numpy array (zeroed on return)."""
        assert dct_coeffs.dtype == np.int16 and dct_coeffs.size >= 128
        _lib.check(self._L.thip_state_frag_recon(self._h, fragi, pli, dct_coeffs.ctypes.data, last_zzi,
                                                 dc_quant, refi, mv), "state_frag_recon")

    def frag_recon_levels(self, fragi, pli, levels, last_zzi, dc_quant, qii, refi, mv):
        """thip_state_frag_recon_levels: `levels` is an int16[128] numpy array holding the quantised levels (zeroed on return)."""
        assert levels.dtype == np.int16 and levels.size >= 128
        _lib.check(self._L.thip_state_frag_recon_levels(self._h, fragi, pli, levels.ctypes.data, last_zzi, dc_quant, qii, refi, mv),
                   "state_frag_recon_levels")

    def frame_dequant_table(self, sel, table_zz):
        t = np.ascontiguousarray(table_zz, np.uint16)
        assert t.size == 64
        _lib.check(self._L.thip_frame_dequant_table(self._h, sel, t.ctypes.data), "frame_dequant_table")

    def frag_copy_list(self, fragis):
        a = np.ascontiguousarray(fragis, np.int64)
        _lib.check(self._L.thip_frag_copy_list(self._h, a.ctypes.data, a.size), "frag_copy_list")

    def loop_filter_frag_rows(self, flimit, refi, pli, fragy0, fragy_end):
        _lib.check(self._L.thip_state_loop_filter_frag_rows(self._h, flimit, refi, pli, fragy0, fragy_end),
                   "loop_filter_frag_rows")

    def frame_flush(self):
        return _lib.check(self._L.thip_frame_flush(self._h), "frame_flush")


# ---------------------------------------------------------------------------------------
# pictures that stay on the device (thip_picture_out)
# ---------------------------------------------------------------------------------------
PIC_FORMATS = {"ycbcr": _lib.PIC_YCBCR, "rgb": _lib.PIC_RGB24, "rgba": _lib.PIC_RGBA32, "rgb_planar": _lib.PIC_RGB_PLANAR}
CHROMA_MODES = {"nearest": _lib.CHROMA_NEAREST, "linear": _lib.CHROMA_LINEAR}


def picture_shapes(fmt, width, height, x=0, pixel_fmt=PF_420, y=0):
    """The output shapes of a width x height picture at (x, y): one (H, W, 3) / (H, W, 4) / (3, H, W) shape, or three plane
    shapes for "ycbcr" (the chroma rectangle by the raw rule of include/theora_hip.h)."""
    if fmt == "rgb":
        return (height, width, 3)
    if fmt == "rgba":
        return (height, width, 4)
    if fmt == "rgb_planar":
        return (3, height, width)
    if fmt != "ycbcr":
        raise ValueError("unknown picture format %r" % (fmt,))
    hdec, vdec = int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))
    cw = ((x + width + hdec) >> hdec) - (x >> hdec)
    ch = ((y + height + vdec) >> vdec) - (y >> vdec)
    return [(height, width), (ch, cw), (ch, cw)]


def _pic_dst(fmt, out, shapes, dtype=None):
    """Destination pointers and row pitches (bytes) of `out` after checking it against the request's shapes (the library writes
    exactly that many rows of that many bytes: a tensor too small for them is refused here).  dtype: the elements, default uint8."""
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    if fmt in ("ycbcr", "rgb_planar"):
        planes = list(out) if isinstance(out, (list, tuple)) else [out[0], out[1], out[2]]
        pshapes = shapes if fmt == "ycbcr" else [shapes[1:]] * 3
        if len(planes) != 3:
            raise ValueError("%s wants three planes" % fmt)
    else:
        planes, pshapes = [out], [shapes]
    ptrs, pitches = [], []
    for t, shp in zip(planes, pshapes):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda:
            raise TypeError("picture destinations are %s device tensors" % str(dtype).replace("torch.", ""))
        if tuple(t.shape) != tuple(shp):
            raise ValueError("destination of shape %s for a picture of %s" % (tuple(t.shape), tuple(shp)))
        if t.stride(-1) != 1 or (t.dim() == 3 and t.stride(1) != t.shape[2]) or t.stride(0) < t.shape[1] * (t.shape[2] if t.dim() == 3 else 1):
            raise ValueError("picture destinations need contiguous rows (a row pitch of their own is fine)")
        ptrs.append(t.data_ptr())
        pitches.append(t.stride(0) * t.element_size())
    while len(ptrs) < 3:
        ptrs.append(None)
        pitches.append(0)
    return ptrs, pitches


_side_streams = {}


def _on_stream(device, stream, call):
    """call(handle) with a hipStream_t that orders like `stream` (default: torch's current stream of `device`).  torch's null
    stream has handle 0, which the library reads as "the state's own stream": such a call goes down a side stream that waits for
    the null stream's work, and the null stream waits for the call's."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    h = s.cuda_stream if hasattr(s, "cuda_stream") else int(s)
    if h:
        return call(h)
    side = _side_streams.get(device)
    if side is None:
        side = _side_streams[device] = torch.cuda.Stream(device)
    side.wait_stream(s)
    rc = call(side.cuda_stream)
    s.wait_stream(side)
    return rc


def picture_out(states, outs, fmt="rgb", chroma="linear", rects=None, bufis=None, stream=None):
    """thip_picture_out: the pictures of `states` into `outs` (uint8 device tensors: (H, W, 3) for "rgb", (H, W, 4) for "rgba",
    (3, H, W) or three (H, W) planes for "rgb_planar", three planes for "ycbcr"); fmt and chroma may be lists, one per state.  rects: per state (x, y, width, height) in
    display coordinates, or None for the whole coded frame; bufis: per state -1 (the newest picture, post-processed if it was)
    or a ring buffer 0..2.  Asynchronous on `stream` (default torch.cuda.current_stream of the states' device)."""
    L = _lib.load()
    n = len(states)
    if len(outs) != n:
        raise ValueError("one destination per state")
    fmts = [fmt] * n if isinstance(fmt, str) else list(fmt)
    chromas = [chroma] * n if isinstance(chroma, str) else list(chroma)
    for f, c in zip(fmts, chromas):
        if f not in PIC_FORMATS or c not in CHROMA_MODES:
            raise ValueError("format %r / chroma %r" % (f, c))
    reqs = (_lib.PictureReq * max(n, 1))()
    for i, st in enumerate(states):
        fmt, chroma = fmts[i], chromas[i]
        x, y, w, h = rects[i] if rects is not None and rects[i] is not None else (0, 0, 0, 0)
        sw, sh = (w, h) if (w or h) else (st.frame_width, st.frame_height)
        ptrs, pitches = _pic_dst(fmt, outs[i], picture_shapes(fmt, sw, sh, x, st.pixel_fmt, y))
        r = reqs[i]
        r.state = st.handle
        r.bufi = -1 if bufis is None else int(bufis[i])
        r.format, r.chroma = PIC_FORMATS[fmt], CHROMA_MODES[chroma]
        r.x, r.y, r.width, r.height = x, y, w, h
        for p in range(3):
            r.dst[p] = ptrs[p]
            r.dst_pitch[p] = pitches[p]
    if n == 0:
        return
    device = states[0].device
    _lib.check(_on_stream(device, stream, lambda h: L.thip_picture_out(reqs, n, h)), "thip_picture_out")


# ---------------------------------------------------------------------------------------
# pictures at another size (thip_picture_resize)
# ---------------------------------------------------------------------------------------
FILTERS = {"bilinear": _lib.FILTER_BILINEAR, "area": _lib.FILTER_AREA}


def picture_resize_shapes(fmt, out_width, out_height, pixel_fmt=PF_420):
    """The output shapes of thip_picture_resize: one (H, W, 3) / (H, W, 4) / (3, H, W) shape, or for "ycbcr" three plane shapes --
    the picture-sized planes Encoder.encode takes for an out_width x out_height picture at offset 0."""
    return picture_shapes(fmt, out_width, out_height, 0, pixel_fmt, 0)


def _elem(dtype):
    import torch
    elems = {torch.uint8: _lib.ELEM_U8, torch.float16: _lib.ELEM_F16, torch.float32: _lib.ELEM_F32}
    if dtype not in elems:
        raise TypeError("picture elements are uint8, float16 or float32, not %r" % (dtype,))
    return elems[dtype]


def picture_resize(states, outs, sizes, fmt="rgb_planar", filter="area", rects=None, bufis=None, dtype=None, scale=None, bias=None,
                   stream=None):
    """thip_picture_resize: per state the rectangle rects[i] (None: the whole coded frame) of its picture resampled to
    sizes[i] = (out_width, out_height) and written to outs[i], device tensors of picture_resize_shapes' shapes.  fmt, filter and
    dtype may be lists, one per state; dtype is torch.uint8 (the default), or with "rgb_planar" torch.float16 / torch.float32:
    the element is then c * scale[k] + bias[k] for channel k (scale and bias: three floats each, default 1 and 0; the same for
    every state).  bufis, stream: as picture_out."""
    import torch
    L = _lib.load()
    n = len(states)
    if len(outs) != n or len(sizes) != n:
        raise ValueError("one destination and one size per state")
    fmts = [fmt] * n if isinstance(fmt, str) else list(fmt)
    filters = [filter] * n if isinstance(filter, str) else list(filter)
    dtypes = list(dtype) if isinstance(dtype, (list, tuple)) else [torch.uint8 if dtype is None else dtype] * n
    scale = (1.0, 1.0, 1.0) if scale is None else tuple(scale)
    bias = (0.0, 0.0, 0.0) if bias is None else tuple(bias)
    if len(scale) != 3 or len(bias) != 3:
        raise ValueError("scale and bias hold one value per channel")
    for f, fl in zip(fmts, filters):
        if f not in PIC_FORMATS or fl not in FILTERS:
            raise ValueError("format %r / filter %r" % (f, fl))
    reqs = (_lib.PictureResizeReq * max(n, 1))()
    for i, st in enumerate(states):
        x, y, w, h = rects[i] if rects is not None and rects[i] is not None else (0, 0, 0, 0)
        ow, oh = sizes[i]
        ptrs, pitches = _pic_dst(fmts[i], outs[i], picture_resize_shapes(fmts[i], ow, oh, st.pixel_fmt), dtypes[i])
        r = reqs[i]
        r.state = st.handle
        r.bufi = -1 if bufis is None else int(bufis[i])
        r.format, r.filter, r.elem = PIC_FORMATS[fmts[i]], FILTERS[filters[i]], _elem(dtypes[i])
        r.x, r.y, r.width, r.height = x, y, w, h
        r.out_width, r.out_height = ow, oh
        for p in range(3):
            r.scale[p], r.bias[p] = scale[p], bias[p]
            r.dst[p] = ptrs[p]
            r.dst_pitch[p] = pitches[p]
    if n == 0:
        return
    _lib.check(_on_stream(states[0].device, stream, lambda h: L.thip_picture_resize(reqs, n, h)), "thip_picture_resize")


# ---------------------------------------------------------------------------------------
# picture metrics (thip_picture_compare)
# ---------------------------------------------------------------------------------------
METRICS = {"sse": _lib.CMP_SSE, "ssim": _lib.CMP_SSIM}


def _cmp_flags(metrics):
    if isinstance(metrics, int):
        return metrics
    names = [metrics] if isinstance(metrics, str) else list(metrics)
    for m in names:
        if m not in METRICS:
            raise ValueError("unknown metric %r" % (m,))
    return sum(METRICS[m] for m in set(names))


def psnr(sse, samples):
    """dump_psnr's formula: 10 (log10(255^2) + log10(samples) - log10(sse)); inf for sse == 0."""
    import math
    if samples <= 0:
        return float("nan")
    if sse <= 0:
        return float("inf")
    return 10.0 * (math.log10(255.0 * 255.0) + math.log10(samples) - math.log10(sse))


def metrics_dict(rec):
    """A thip_picture_metrics record (12 int64 values: a tensor, array or list; sse, samples, ssim_q20, windows by plane) as a dict:
    sse, samples, ssim_q20, windows (lists by plane), psnr (by plane, then over the three planes' sums: dump_psnr's numbers) and
    ssim (ssim_q20 / windows / 2^20 by plane; None for a plane without windows).  A device tensor is read here (a host wait)."""
    v = [int(t) for t in (rec.tolist() if hasattr(rec, "tolist") else rec)]
    sse, samples, q20, win = v[0:3], v[3:6], v[6:9], v[9:12]
    return dict(sse=sse, samples=samples, ssim_q20=q20, windows=win,
                psnr=[psnr(e, n) for e, n in zip(sse, samples)] + [psnr(sum(sse), sum(samples))],
                ssim=[q / n / float(1 << 20) if n else None for q, n in zip(q20, win)])


def picture_compare(states, refs, results, metrics=("sse",), rects=None, bufis=None, blocks=None, stream=None):
    """thip_picture_compare: per state the rectangle rects[i] (None: the whole coded frame) of its picture against refs[i], three
    uint8 device planes of picture_shapes("ycbcr", ...)'s shapes for that rectangle (rows may have a pitch of their own).
    results[i]: an int64 device tensor of 12 elements, overwritten with thip_picture_metrics (metrics_dict reads it).  metrics:
    "sse", "ssim" or both (or the THIP_CMP_* flags).  blocks[i]: None, or three 2-D int32 device tensors of (rows + 7) // 8 by
    (columns + 7) // 8 elements that take block_sse.  bufis, stream: as picture_out."""
    import torch
    L = _lib.load()
    n = len(states)
    if len(refs) != n or len(results) != n:
        raise ValueError("one reference picture and one result per state")
    flags = _cmp_flags(metrics)
    reqs = (_lib.PictureCompareReq * max(n, 1))()
    for i, st in enumerate(states):
        x, y, w, h = rects[i] if rects is not None and rects[i] is not None else (0, 0, 0, 0)
        fw, fh = (w, h) if (w or h) else (st.frame_width, st.frame_height)
        shapes = picture_shapes("ycbcr", fw, fh, x if (w or h) else 0, st.pixel_fmt, y if (w or h) else 0)
        r = reqs[i]
        r.state = st.handle
        r.bufi = -1 if bufis is None else int(bufis[i])
        r.flags = flags
        r.x, r.y, r.width, r.height = x, y, w, h
        for p in range(3):
            t = refs[i][p]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
                raise TypeError("reference pictures are uint8 device tensors")
            if tuple(t.shape) != tuple(shapes[p]) or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
                raise ValueError("reference plane %d of shape %s for a plane of %s" % (p, tuple(t.shape), tuple(shapes[p])))
            r.ref[p], r.ref_pitch[p] = t.data_ptr(), t.stride(0)
        res = results[i]
        if not isinstance(res, torch.Tensor) or res.dtype != torch.int64 or not res.is_cuda or res.numel() != 12 or not res.is_contiguous():
            raise TypeError("a result is a contiguous int64 device tensor of 12 elements")
        r.result = res.data_ptr()
        if blocks is not None and blocks[i] is not None:
            for p in range(3):
                b = blocks[i][p]
                want = ((shapes[p][0] + 7) // 8, (shapes[p][1] + 7) // 8)
                if not isinstance(b, torch.Tensor) or b.dtype != torch.int32 or not b.is_cuda or b.dim() != 2 or b.stride(1) != 1:
                    raise TypeError("block sums go to 2-D int32 device tensors")
                if tuple(b.shape) != want:
                    raise ValueError("block tensor of shape %s for %s blocks" % (tuple(b.shape), want))
                r.block_sse[p], r.block_pitch[p] = b.data_ptr(), b.stride(0)
    if n == 0:
        return
    _lib.check(_on_stream(states[0].device, stream, lambda h: L.thip_picture_compare(reqs, n, h)), "thip_picture_compare")


# ---------------------------------------------------------------------------------------
# frame side data (thip_frame_info_out)
# ---------------------------------------------------------------------------------------
FI_REFS = {"prev": _lib.FI_REF_PREV, "gold": _lib.FI_REF_GOLD}
FI_OUTPUTS = ("kind", "mv", "ncoef", "flow", "valid")


def frame_info_shapes(width, height, x=0, y=0, pixel_fmt=PF_420):
    """The output shapes of thip_frame_info_out for the rectangle (x, y, width, height) of a coded frame, display coordinates:
    {"kind": three (rows, cols), "mv": three (rows, cols, 2), "ncoef": three (rows, cols), "flow": (2, height, width),
    "valid": (height, width)}.  The maps of plane p cover the fragments the rectangle touches: columns (x >> hdec_p) >> 3 ..
    ((x + width - 1) >> hdec_p) >> 3, rows likewise with vdec_p (include/theora_hip.h)."""
    if width < 1 or height < 1 or x < 0 or y < 0:
        raise ValueError("an empty or negative rectangle")
    hdec, vdec = int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))
    frags = []
    for p in range(3):
        hd, vd = (hdec, vdec) if p else (0, 0)
        frags.append(((((y + height - 1) >> vd) >> 3) - ((y >> vd) >> 3) + 1, (((x + width - 1) >> hd) >> 3) - ((x >> hd) >> 3) + 1))
    return dict(kind=list(frags), mv=[f + (2,) for f in frags], ncoef=list(frags), flow=(2, height, width), valid=(height, width))


def _fi_refs(refs):
    if isinstance(refs, int):
        return refs
    names = [refs] if isinstance(refs, str) else list(refs)
    for r in names:
        if r not in FI_REFS:
            raise ValueError("unknown reference %r" % (r,))
    return sum(FI_REFS[r] for r in set(names))


def frame_info(states, outs, rects=None, refs=("prev",), frag_infos=None, stream=None):
    """thip_frame_info_out: per state the side data of a frame into outs[i], a dict with any of the keys "kind", "mv", "ncoef"
    (three device tensors each, one per plane; an entry may be None), "flow" and "valid", of frame_info_shapes' shapes: uint8 for
    kind, ncoef and valid, int8 for mv, float16 or float32 for flow (rows may have a pitch of their own).  rects: per state
    (x, y, width, height) in display coordinates, None: the whole coded frame.  refs: "prev", "gold", both (or the THIP_FI_REF_*
    flags): the kinds whose vectors flow holds; may be a list of such, one per state.  frag_infos: per state a device tensor
    holding a frame's frag_info words in tile order (info_words' layout), or None for the state's own record
    (State.set_frame_info).  Asynchronous on `stream` (default torch.cuda.current_stream of the states' device)."""
    import torch
    L = _lib.load()
    n = len(states)
    if len(outs) != n or (frag_infos is not None and len(frag_infos) != n) or (rects is not None and len(rects) != n):
        raise ValueError("one destination, rectangle and frag_info per state")
    per_state = isinstance(refs, list) and len(refs) == n and all(isinstance(r, (tuple, list, int)) for r in refs)
    reqs = (_lib.FrameInfoReq * max(n, 1))()
    keep = []
    for i, st in enumerate(states):
        x, y, w, h = rects[i] if rects is not None and rects[i] is not None else (0, 0, 0, 0)
        rw, rh = (w, h) if (w or h) else (st.frame_width, st.frame_height)
        shapes = frame_info_shapes(rw, rh, x if (w or h) else 0, y if (w or h) else 0, st.pixel_fmt)
        r = reqs[i]
        r.state = st.handle
        fi = frag_infos[i] if frag_infos is not None else None
        if fi is not None:
            if not isinstance(fi, torch.Tensor) or not fi.is_cuda or not fi.is_contiguous() or fi.element_size() != 4 or fi.numel() != 2 * 64 * st.ntiles:
                raise ValueError("frag_info is a contiguous device tensor of 2 * 64 * ntiles 32-bit words")
            keep.append(fi)
            r.frag_info = fi.data_ptr()
        r.x, r.y, r.width, r.height = x, y, w, h
        r.refs = _fi_refs(refs[i] if per_state else refs)
        out = outs[i]
        for key in out:
            if key not in FI_OUTPUTS:
                raise ValueError("unknown output %r" % (key,))

        def plane(t, shape, dtypes, what):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes:
                raise TypeError("%s goes to a %s device tensor" % (what, " or ".join(str(d).replace("torch.", "") for d in dtypes)))
            if tuple(t.shape) != tuple(shape) or t.stride(-1) != 1:
                raise ValueError("%s of shape %s for %s" % (what, tuple(t.shape), tuple(shape)))
            return t
        for key, dt in (("kind", torch.uint8), ("ncoef", torch.uint8), ("mv", torch.int8)):
            ts = out.get(key)
            if ts is None:
                continue
            if len(ts) != 3:
                raise ValueError("%s wants three planes (None for one not wanted)" % key)
            for p in range(3):
                if ts[p] is None:
                    continue
                t = plane(ts[p], shapes[key][p], (dt,), key)
                if key == "mv" and t.stride(1) != 2:
                    raise ValueError("mv keeps a fragment's two bytes together")
                getattr(r, key)[p] = t.data_ptr()
                getattr(r, key + "_pitch")[p] = t.stride(0)
        t = out.get("flow")
        if t is not None:
            t = plane(t, shapes["flow"], (torch.float16, torch.float32), "flow")
            if t.stride(0) != t.shape[1] * t.stride(1):
                raise ValueError("flow's second plane follows the first at height rows")
            r.flow, r.flow_pitch, r.elem = t.data_ptr(), t.stride(1) * t.element_size(), _elem(t.dtype)
        t = out.get("valid")
        if t is not None:
            t = plane(t, shapes["valid"], (torch.uint8,), "valid")
            r.valid, r.valid_pitch = t.data_ptr(), t.stride(0)
    if n == 0:
        return
    _lib.check(_on_stream(states[0].device, stream, lambda h: L.thip_frame_info_out(reqs, n, h)), "thip_frame_info_out")


def frame_info_alloc(shapes, what, dtype, device):
    """Fresh device tensors for the outputs `what` of frame_info_shapes' `shapes`: the dict frame_info takes."""
    import torch
    out = {}
    for key in what:
        if key not in FI_OUTPUTS:
            raise ValueError("unknown output %r" % (key,))
        if key == "flow":
            out[key] = torch.empty(shapes[key], dtype=dtype, device=device)
        elif key == "valid":
            out[key] = torch.empty(shapes[key], dtype=torch.uint8, device=device)
        else:
            out[key] = [torch.empty(s, dtype=torch.int8 if key == "mv" else torch.uint8, device=device) for s in shapes[key]]
    return out


# ---------------------------------------------------------------------------------------
# R'G'B' pictures in (thip_picture_in)
# ---------------------------------------------------------------------------------------
def picture_in_shapes(width, height, pixel_fmt=PF_420, pic_x=0, pic_y=0):
    """The three plane shapes thip_picture_in writes for a width x height picture at (pic_x, pic_y) of its coded frame: luma
    (height, width), chroma the region of spec 4.4 (include/theora_hip.h) -- the picture-sized planes Encoder.encode takes."""
    hdec, vdec = int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))
    cw = ((pic_x + width + hdec) >> hdec) - (pic_x >> hdec)
    ch = ((pic_y + height + vdec) >> vdec) - (pic_y >> vdec)
    return [(height, width), (ch, cw), (ch, cw)]


def _pic_src(fmt, src):
    """(width, height, pointers, row pitches) of an R'G'B' source: a uint8 device tensor (H, W, 3) for "rgb", (H, W, 4) for
    "rgba", (3, H, W) or three (H, W) planes for "rgb_planar"; rows may have a pitch of their own, pixels are contiguous."""
    import torch
    if fmt == "rgb_planar":
        planes = list(src) if isinstance(src, (list, tuple)) else [src[0], src[1], src[2]]
        if len(planes) != 3:
            raise ValueError("rgb_planar wants three planes")
    elif fmt in ("rgb", "rgba"):
        planes = [src]
    else:
        raise ValueError("unknown R'G'B' format %r" % (fmt,))
    want = {"rgb": (3, 3), "rgba": (3, 4), "rgb_planar": (2, 0)}[fmt]
    ptrs, pitches = [], []
    for t in planes:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
            raise TypeError("picture sources are uint8 device tensors")
        if t.dim() != want[0] or (want[1] and t.shape[2] != want[1]) or tuple(t.shape[:2]) != tuple(planes[0].shape[:2]):
            raise ValueError("a source of shape %s for format %r" % (tuple(t.shape), fmt))
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("an empty picture")
        if t.stride(-1) != 1 or (t.dim() == 3 and t.stride(1) != t.shape[2]) or t.stride(0) < t.shape[1] * (t.shape[2] if t.dim() == 3 else 1):
            raise ValueError("picture sources need contiguous rows (a row pitch of their own is fine)")
        ptrs.append(t.data_ptr())
        pitches.append(t.stride(0))
    while len(ptrs) < 3:
        ptrs.append(None)
        pitches.append(0)
    return planes[0].shape[1], planes[0].shape[0], ptrs, pitches


def picture_in(srcs, pixel_fmt, fmt="rgb", pics=None, outs=None, stream=None):
    """thip_picture_in: the R'G'B' pictures `srcs` (see _pic_src for their shapes; fmt may be a list, one per source, and so may
    pixel_fmt) as Y'CbCr planes.  pics: per source (pic_x, pic_y), where the picture sits in its coded frame (default (0, 0));
    outs: per source three uint8 device tensors of picture_in_shapes' shapes (rows may have a pitch of their own), made here
    when None.  Returns the three planes per source.  Asynchronous on `stream` (default torch.cuda.current_stream of the
    sources' device)."""
    import torch
    L = _lib.load()
    n = len(srcs)
    fmts = [fmt] * n if isinstance(fmt, str) else list(fmt)
    pfs = [pixel_fmt] * n if isinstance(pixel_fmt, int) else list(pixel_fmt)
    if len(fmts) != n or len(pfs) != n or (outs is not None and len(outs) != n) or (pics is not None and len(pics) != n):
        raise ValueError("one format, pixel format, offset and destination per source")
    if n == 0:
        return []
    reqs = (_lib.PictureInReq * n)()
    res, device = [], None
    for i in range(n):
        w, h, ptrs, pitches = _pic_src(fmts[i], srcs[i])
        dev = (srcs[i][0] if isinstance(srcs[i], (list, tuple)) else srcs[i]).device
        if device is None:
            device = dev
        elif dev != device:
            raise ValueError("all sources of a call live on one device")
        px, py = pics[i] if pics is not None and pics[i] is not None else (0, 0)
        shapes = picture_in_shapes(w, h, pfs[i], px, py)
        if outs is None or outs[i] is None:
            out = [torch.empty(sh, dtype=torch.uint8, device=device) for sh in shapes]
        else:
            out = list(outs[i])
            for t, sh in zip(out, shapes):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != device:
                    raise TypeError("picture destinations are uint8 tensors on the sources' device")
                if tuple(t.shape) != tuple(sh) or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
                    raise ValueError("a destination of shape %s for a plane of %s" % (tuple(t.shape), tuple(sh)))
        r = reqs[i]
        r.format, r.pixel_fmt = PIC_FORMATS[fmts[i]], pfs[i]
        r.pic_x, r.pic_y, r.width, r.height = px, py, w, h
        for p in range(3):
            r.src[p], r.src_pitch[p] = ptrs[p], pitches[p]
            r.dst[p], r.dst_pitch[p] = out[p].data_ptr(), out[p].stride(0)
        res.append(out)
    s = stream if stream is not None else torch.cuda.current_stream(device)
    with torch.cuda.device(device):   # (the call runs on the calling thread's current device)
        _lib.check(L.thip_picture_in(reqs, n, s.cuda_stream), "thip_picture_in")
    return res


def decode_frames(states, descs, stream=None):
    """thip_decode_frames over parallel lists of State and FrameDesc; returns per-stream results."""
    L = _lib.load()
    n = len(states)
    assert n == len(descs)
    hs = (C.c_void_p * n)(*[s.handle for s in states])
    ds = (FrameDesc * n)(*descs)
    res = (C.c_int32 * n)()
    _lib.check(L.thip_decode_frames(hs, ds, n, stream, res), "thip_decode_frames")
    return list(res)


class BatchPlan:
    """A pre-marshalled thip_decode_frames call (bench.py's timed loop reuses these so the
    Python/ctypes overhead per step is one foreign call)."""

    def __init__(self, states, descs):
        self._L = _lib.load()
        self.n = len(states)
        self.hs = (C.c_void_p * self.n)(*[s.handle for s in states])
        self.ds = (FrameDesc * self.n)(*descs)
        self.res = (C.c_int32 * self.n)()

    def submit(self, stream=None):
        rc = self._L.thip_decode_frames(self.hs, self.ds, self.n, stream, self.res)
        if rc < 0:
            raise TheoraHipError("thip_decode_frames failed: %d" % rc)


def synchronize():
    """thip_synchronize: waits for the library's streams; raises while some state's fault word is set (it only reports: the state's
    own State.check_fault() / ycbcr_out / read_plane repair or clear it)."""
    _lib.check(_lib.load().thip_synchronize(), "thip_synchronize")


def make_desc(info_dev, coeffs_dev, slot0_dev, nslots, ncoded, frame_type, flimit, dc_tokens_dev=None, dequant_dev=None):
    """dequant_dev given: the LEVELS form (coeffs_dev = units, slot0 = first units | SLOT_WIDE, nslots = units)."""
    return FrameDesc(_ptr(info_dev), _ptr(coeffs_dev), _ptr(slot0_dev), nslots, ncoded, frame_type, flimit,
                     _ptr(dc_tokens_dev), COEFFS_LEVELS if dequant_dev is not None else COEFFS_DEQUANT16, _ptr(dequant_dev))


def profile_enable(on):
    _lib.check(_lib.load().thip_profile_enable(int(on)), "profile_enable")


def profile_reset():
    _lib.check(_lib.load().thip_profile_reset(), "profile_reset")


def profile_read():
    n = (C.c_int64 * _lib.NKERNELS)()
    ms = (C.c_double * _lib.NKERNELS)()
    _lib.check(_lib.load().thip_profile_read(n, ms), "profile_read")
    return list(n), list(ms)


# ---------------------------------------------------------------------------------------
# batched single slots (device tensors in, device tensors out)
# ---------------------------------------------------------------------------------------
def idct8x8_batch(x_dev, last_zzi_dev=None):
    import torch
    y = torch.empty_like(x_dev)
    n = x_dev.numel() // 64
    _lib.check(_lib.load().thip_idct8x8_batch(_ptr(y), _ptr(x_dev), _ptr(last_zzi_dev), n), "idct8x8_batch")
    return y


def fdct8x8_batch(x_dev):
    import torch
    y = torch.empty_like(x_dev)
    _lib.check(_lib.load().thip_enc_fdct8x8_batch(_ptr(y), _ptr(x_dev), x_dev.numel() // 64), "fdct8x8_batch")
    return y


def enc_quantize_batch(dct_dev, dequant_dev):
    """oc_enc_quantize over [n,64] zig-zag-ordered int16 blocks; returns (qdct, nonzero)."""
    import torch
    n = dct_dev.numel() // 64
    q = torch.empty_like(dct_dev)
    nz = torch.empty(n, dtype=torch.int32, device=dct_dev.device)
    _lib.check(_lib.load().thip_enc_quantize_batch(_ptr(q), _ptr(nz), _ptr(dct_dev), _ptr(dequant_dev), n),
               "enc_quantize_batch")
    return q, nz


def enc_fdct_quantize_batch(x_dev, dequant_dev, want_dct=False):
    """thip_enc_fdct_quantize_batch over [n,64] natural-order int16 residual blocks; returns (qdct, nonzero[, dct])."""
    import torch
    n = x_dev.numel() // 64
    q = torch.empty_like(x_dev)
    nz = torch.empty(n, dtype=torch.int32, device=x_dev.device)
    dct = torch.empty_like(x_dev) if want_dct else None
    _lib.check(_lib.load().thip_enc_fdct_quantize_batch(_ptr(q), _ptr(nz), _ptr(dct), _ptr(x_dev), _ptr(dequant_dev), None, n),
               "enc_fdct_quantize_batch")
    return (q, nz, dct) if want_dct else (q, nz)


def enc_metric_batch(op, src_plane, ref_plane, ystride, src_offs, ref_offs=None, ref2_offs=None, thresh=0):
    import torch
    n = src_offs.numel()
    out = torch.empty(n, dtype=torch.int32, device=src_offs.device)
    dc = torch.empty(n, dtype=torch.int32, device=src_offs.device)   # (the kernel writes every element: 0 for the SAD family)
    _lib.check(_lib.load().thip_enc_frag_metric_batch(
        _lib.ENC_OPS[op], _ptr(out), _ptr(dc), _ptr(src_plane), _ptr(ref_plane), ystride, _ptr(src_offs),
        _ptr(ref_offs), _ptr(ref2_offs), thresh, n), "enc_frag_metric_batch")
    return out, dc


def enc_mb_cost_maps(planes, frame_width, frame_height, pixel_fmt):
    """thip_enc_mb_cost_maps over three device planes ([H, stride] uint8 tensors, bitstream row order).  Returns
    (intra_satd [nmbs,12], luma [nmbs], activity [nmbs,4], activity_fast [nmbs,4]) as int32 device tensors."""
    import torch
    L = _lib.load()
    nmbs = L.thip_enc_mb_count(frame_width, frame_height)
    dev = planes[0].device
    satd = torch.empty((nmbs, 12), dtype=torch.int32, device=dev)
    luma = torch.empty(nmbs, dtype=torch.int32, device=dev)
    act = torch.empty((nmbs, 4), dtype=torch.int32, device=dev)
    fast = torch.empty((nmbs, 4), dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * 3)(*[_ptr(p) for p in planes])
    strides = (C.c_int32 * 3)(*[int(p.stride(0)) for p in planes])
    _lib.check(L.thip_enc_mb_cost_maps(ptrs, strides, frame_width, frame_height, pixel_fmt, _ptr(satd), _ptr(luma), _ptr(act),
                                       _ptr(fast)), "enc_mb_cost_maps")
    return satd, luma, act, fast


def enc_metric_halfpel_batch(op, src_plane, ref_plane, ystride, src_offs, ref_offs, vecs, sites):
    """thip_enc_frag_metric_halfpel_batch: every block against the half-pel vectors 2 * vec + (dx, dy), `sites` = [(dx, dy), ...]
    without (0, 0), around its whole-pel vector (vecs: int16 tensor, x & 0xFF | y << 8; ref_offs: the block at that vector).
    op "satd2" or "sad2_thresh".  Returns (values, dc), both [len(sites), nblocks]; dc is None for "sad2_thresh"."""
    import numpy as np
    import torch
    n = src_offs.numel()
    ns = len(sites)
    out = torch.empty((ns, n), dtype=torch.int32, device=src_offs.device)
    dc = torch.empty((ns, n), dtype=torch.int32, device=src_offs.device) if op == "satd2" else None
    dx = np.array([s[0] for s in sites], np.int8)
    dy = np.array([s[1] for s in sites], np.int8)
    _lib.check(_lib.load().thip_enc_frag_metric_halfpel_batch(
        _lib.ENC_OPS[op], _ptr(out), _ptr(dc), _ptr(src_plane), _ptr(ref_plane), ystride, _ptr(src_offs), _ptr(ref_offs), _ptr(vecs),
        dx.ctypes.data, dy.ctypes.data, ns, n), "enc_frag_metric_halfpel_batch")
    return out, dc


def enc_metric_sites_batch(op, src_plane, ref_plane, ystride, src_offs, ref_offs, sites):
    """thip_enc_frag_metric_sites_batch: every block against the candidate positions `sites` = [(dx, dy), ...] around its
    reference position.  Returns (values, dc), both [len(sites), nblocks] (candidate-major); dc is None for "sad"."""
    import numpy as np
    import torch
    n = src_offs.numel()
    ns = len(sites)
    out = torch.empty((ns, n), dtype=torch.int32, device=src_offs.device)
    dc = torch.empty((ns, n), dtype=torch.int32, device=src_offs.device) if op == "satd" else None
    dx = np.array([s[0] for s in sites], np.int8)
    dy = np.array([s[1] for s in sites], np.int8)
    _lib.check(_lib.load().thip_enc_frag_metric_sites_batch(
        _lib.ENC_OPS[op], _ptr(out), _ptr(dc), _ptr(src_plane), _ptr(ref_plane), ystride, _ptr(src_offs), _ptr(ref_offs),
        dx.ctypes.data, dy.ctypes.data, ns, n), "enc_frag_metric_sites_batch")
    return out, dc
