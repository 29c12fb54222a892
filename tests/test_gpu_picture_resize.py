"""Resized pictures on the device (thip_picture_resize / TH_DECCTL_THIP_PICTURE_RESIZE, k_picture_resize): bit-exact against the
numpy restatement of the definition (tests/picture_resize_ref.py) applied to State.ycbcr_out() / Decoder.ycbcr_out(), which the
other GPU tests check against the oracle; plus float bit patterns, awkward destinations, chunking, ordering, the refusals and the
transcoding chain into the encoder."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import picture_resize_ref as rr, streamgen

pytestmark = pytest.mark.gpu

FORMATS = ["ycbcr", "rgb", "rgba", "rgb_planar"]
FILTERS = ["bilinear", "area"]
SCALE = [1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225)]     # (c / 255 - mean) / std as c * scale + bias
BIAS = [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]
CANARY = 0xA5


def _state(hip, w, h, fmt, seed):
    """A state whose newest frame is random content written into buffer 0."""
    st = hip.State(w, h, fmt)
    rng = np.random.default_rng(seed)
    for pli in range(3):
        g = st.planes[pli]
        st.write_plane(0, pli, rng.integers(0, 256, (g["height"], g["width"]), dtype=np.uint8))
    st.set_ref_idx(0, 0, 0)
    return st


def _host(out):
    if isinstance(out, (tuple, list)):
        return [o.cpu().numpy() for o in out]
    return out.cpu().numpy()


def _bits(a):
    """Float arrays as integers of their width: the comparison is of bit patterns."""
    a = np.asarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want):
    if isinstance(want, list):
        return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    return np.array_equal(_bits(got), _bits(want))


def _np_dtype(dtype):
    import torch
    return {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}[dtype]


def _want(planes, pf, size, fmt, filt, rect=None, dtype=None):
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    return rr.resize(planes, pf, size, fmt, filt, rect, _np_dtype(dtype), [np.float32(s) for s in SCALE], [np.float32(b) for b in BIAS])


@pytest.mark.parametrize("pf", [0, 2, 3])
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (176, 144)])
def test_every_format_filter_and_size(hip, w, h, pf):
    from theora_amd import TheoraHipError
    st = _state(hip, w, h, pf, w + h + pf)
    planes = st.ycbcr_out()
    rects = [None] + [r for r in [(3, 5, 37, 21), (1, 1, 15, 9)] if r[0] + r[2] <= w and r[1] + r[3] <= h]
    ran = refused = 0
    for rect in rects:
        own = (rect[2], rect[3]) if rect else (w, h)
        for size in [(1, 1), (15, 9), (16, 16), (17, 33), (224, 224), own]:
            for fmt in FORMATS:
                for filt in FILTERS:
                    if rr.refused(planes, pf, fmt, filt, size, rect):
                        # the area limit: only an output one sample wide or high of a source beyond 32 samples
                        assert size == (1, 1) and max(own) > 32, (rect, size, fmt, filt)
                        with pytest.raises(TheoraHipError, match="-10"):
                            st.picture_resized(size, fmt, filt, rect)
                        refused += 1
                        continue
                    got = _host(st.picture_resized(size, fmt, filt, rect))
                    assert _same(got, _want(planes, pf, size, fmt, filt, rect)), (rect, size, fmt, filt)
                    ran += 1
    assert ran + refused == len(rects) * 6 * 8
    assert refused == 4 * sum(1 for r in rects if max((r[2], r[3]) if r else (w, h)) > 32)     # (1, 1), area, the four formats
    st.close()


def test_float_output_bit_patterns(hip):
    import torch
    st = _state(hip, 48, 32, 0, 21)
    planes = st.ycbcr_out()
    for dtype in (torch.float32, torch.float16):
        for filt in FILTERS:
            for size, rect in (((17, 33), None), ((16, 16), (3, 5, 37, 21)), ((48, 32), None), ((224, 224), None)):
                out = st.picture_resized(size, "rgb_planar", filt, rect, dtype=dtype, scale=SCALE, bias=BIAS)
                assert out.dtype == dtype and tuple(out.shape) == (3, size[1], size[0])
                assert _same(_host(out), _want(planes, 0, size, "rgb_planar", filt, rect, dtype)), (dtype, filt, size)
    # scale and bias default to 1 and 0: the 8-bit components themselves
    out = st.picture_resized((20, 10), "rgb_planar", "area", dtype=torch.float32)
    assert np.array_equal(_host(out), rr.resize(planes, 0, (20, 10), "rgb_planar", "area").astype(np.float32))
    st.close()


@functools.lru_cache(maxsize=None)
def _large_planes():
    rng = np.random.default_rng(1088)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((1088, 1920), (544, 960), (544, 960)))


def test_one_large_pair(hip):
    """1080p inside its 1920 x 1088 coded frame to 720p planes for the encoder, and to a 224 x 224 normalised float16 tensor."""
    import torch
    st = hip.State(1920, 1088, 0)
    for pli, p in enumerate(_large_planes()):
        st.write_plane(0, pli, p[::-1])        # (write_plane takes bitstream order: bottom row first)
    st.set_ref_idx(0, 0, 0)
    planes = st.ycbcr_out()
    assert all(np.array_equal(a, b) for a, b in zip(planes, _large_planes()))
    rect = (0, 0, 1920, 1080)
    got = st.picture_resized((1280, 720), "ycbcr", "area", rect)
    assert [tuple(g.shape) for g in got] == [(720, 1280), (360, 640), (360, 640)]
    assert _same(_host(got), _want(planes, 0, (1280, 720), "ycbcr", "area", rect))
    got = st.picture_resized((224, 224), "rgb_planar", "area", rect, dtype=torch.float16, scale=SCALE, bias=BIAS)
    assert _same(_host(got), _want(planes, 0, (224, 224), "rgb_planar", "area", rect, torch.float16))
    st.close()


DEST_CASES = [("ycbcr", "uint8"), ("rgb", "uint8"), ("rgba", "uint8"), ("rgb_planar", "uint8"), ("rgb_planar", "float16"),
              ("rgb_planar", "float32")]


@pytest.mark.parametrize("rect,size", [(None, (33, 17)), ((3, 5, 101, 77), (48, 31))])
def test_awkward_destinations_and_guard_elements(hip, rect, size):
    """Rows with a pitch of their own, bases one element off a 16-byte boundary (1 byte for uint8, 4 for float32): the rectangles
    hold the picture and every byte around them is as it was."""
    import theora_amd
    import torch
    w, h, pf = 176, 144, 0
    st = _state(hip, w, h, pf, 5)
    planes = st.ycbcr_out()
    for filt in FILTERS:
        for fmt, dname in DEST_CASES:
            dtype = getattr(torch, dname)
            want = _want(planes, pf, size, fmt, filt, rect, dtype)
            shp = theora_amd.picture_resize_shapes(fmt, size[0], size[1], pf)
            pshapes = shp if fmt == "ycbcr" else ([shp[1:]] * 3 if fmt == "rgb_planar" else [shp])
            bufs, views = [], []
            for ps in pshapes:
                row = int(np.prod(ps[1:]))                     # elements a row
                pitch = row + (1 if row % 2 == 0 else 2)       # odd
                guard = 64
                buf = torch.empty(2 * guard + 1 + ps[0] * pitch, dtype=dtype, device="cuda")
                buf.view(torch.uint8).fill_(CANARY)
                strides = (pitch,) + ((ps[2], 1) if len(ps) == 3 else (1,))
                views.append(torch.as_strided(buf, ps, strides, guard + 1))
                bufs.append((buf, pitch, row, guard))
            out = views if fmt in ("ycbcr", "rgb_planar") else views[0]
            theora_amd.picture_resize([st], [out], [size], fmt, filt, [rect], dtype=dtype, scale=SCALE, bias=BIAS)
            torch.cuda.synchronize()
            wl = want if fmt == "ycbcr" else (list(want) if fmt == "rgb_planar" else [want])
            for (buf, pitch, row, guard), wp in zip(bufs, wl):
                esz = buf.element_size()
                b = buf.view(torch.uint8).cpu().numpy()
                lo, hi = (guard + 1) * esz, (guard + 1 + wp.shape[0] * pitch) * esz
                body = b[lo:hi].reshape(wp.shape[0], pitch * esz)
                assert np.array_equal(body[:, :row * esz], np.ascontiguousarray(wp).view(np.uint8).reshape(wp.shape[0], row * esz)), (fmt, dname, filt)
                assert (body[:, row * esz:] == CANARY).all(), (fmt, dname, filt)
                assert (b[:lo] == CANARY).all() and (b[hi:] == CANARY).all(), (fmt, dname, filt)
    st.close()


def test_batch_of_nine_is_chunked(hip):
    import theora_amd
    import torch
    geom = [(176, 144, 0), (64, 48, 2), (48, 80, 3), (320, 240, 0), (16, 16, 0), (176, 144, 3), (128, 64, 2), (96, 96, 0), (640, 480, 0)]
    states = [_state(hip, w, h, f, 100 + i) for i, (w, h, f) in enumerate(geom)]
    n = len(states)
    fmts = [FORMATS[i % 4] for i in range(n)]
    filters = [FILTERS[(i // 2) % 2] for i in range(n)]
    dtypes = [torch.float16 if i == 3 else torch.float32 if i == 7 else torch.uint8 for i in range(n)]     # (both rgb_planar)
    sizes = [(33, 17), (16, 16), (100, 90), (224, 224), (5, 7), (31, 64), (128, 64), (48, 48), (320, 200)]
    rects = [None if i % 2 else (3, 5, 11, 9) for i in range(n)]
    assert fmts[3] == fmts[7] == "rgb_planar"
    single = [_host(s.picture_resized(sz, f, fl, r, dtype=d, scale=SCALE, bias=BIAS))
              for s, sz, f, fl, r, d in zip(states, sizes, fmts, filters, rects, dtypes)]
    outs = []
    for s, sz, f, d in zip(states, sizes, fmts, dtypes):
        shp = theora_amd.picture_resize_shapes(f, sz[0], sz[1], s.pixel_fmt)
        outs.append([torch.zeros(p, dtype=d, device="cuda") for p in shp] if f == "ycbcr" else torch.zeros(shp, dtype=d, device="cuda"))
    theora_amd.picture_resize(states, outs, sizes, fmts, filters, rects, dtype=dtypes, scale=SCALE, bias=BIAS)
    for k, (o, want) in enumerate(zip(outs, single)):
        assert _same(_host(o), want), k
    for k, s in enumerate(states):       # ... and the single calls are the definition's
        assert _same(single[k], _want(s.ycbcr_out(), s.pixel_fmt, sizes[k], fmts[k], filters[k], rects[k], dtypes[k])), k
        s.close()


def test_postprocessed_and_as_decoded(hip):
    from theora_amd import _lib
    L = _lib.load()
    w, h, pf = 176, 144, 0
    st = _state(hip, w, h, pf, 7)
    decoded = [st.read_plane(0, p)[::-1] for p in range(3)]
    rng = np.random.default_rng(3)
    n = st.nfrags
    dc_qis = rng.integers(0, 64, n).astype(np.uint8)
    frag_qi = rng.integers(0, 64, n).astype(np.uint8)
    dcs = np.sort(rng.integers(1, 90, 64))[::-1].astype(np.int32).copy()
    shm = (-rng.integers(0, 6, 64)).astype(np.int32)
    assert L.thip_state_postprocess(st.handle, 7, dc_qis.ctypes.data, frag_qi.ctypes.data, dcs.ctypes.data, shm.ctypes.data) == 0
    pp = st.ycbcr_out()
    assert any(not np.array_equal(a, b) for a, b in zip(pp, decoded))   # the filters changed the picture
    for fmt in FORMATS:
        for filt in FILTERS:
            assert _same(_host(st.picture_resized((96, 80), fmt, filt)), _want(pp, pf, (96, 80), fmt, filt)), (fmt, filt)
            assert _same(_host(st.picture_resized((96, 80), fmt, filt, bufi=0)), _want(decoded, pf, (96, 80), fmt, filt)), (fmt, filt)
    st.close()


def _decode(hip, gst, geom, rng, ftype, keep):
    from theora_amd import synth
    fr = synth.gen_frame(geom, rng, ftype, "mixed", flimit=4)
    desc, ka = synth.upload_frame(synth.pack_frame(geom, fr))
    keep.append(ka)
    hip.decode_frames([gst], [desc])


def test_ordering_on_a_torch_stream(hip):
    """A frame decoded after the call does not change what the call wrote."""
    import torch
    from theora_amd import synth
    w, h = 176, 144
    geom = synth.Geometry(w, h)
    rng = np.random.default_rng(11)
    gst = hip.State(w, h)
    keep = []
    _decode(hip, gst, geom, rng, hip.INTRA_FRAME, keep)
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)
    want = _want(gst.ycbcr_out(), 0, (96, 80), "rgba", "area")
    s = torch.cuda.Stream()
    big = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(8):           # keep the stream busy: the picture starts late
            big.add_(1)
        out = gst.picture_resized((96, 80), "rgba", "area", stream=s)
        after = out.clone()          # a torch op behind the call on the same stream
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)   # the second of these writes the buffer the picture reads
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)
    torch.cuda.synchronize()
    hip.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(after.cpu().numpy(), want)
    # torch's default (null) stream
    want = _want(gst.ycbcr_out(), 0, (40, 30), "rgb", "bilinear")
    out = gst.picture_resized((40, 30), "rgb", "bilinear")
    assert out.to(torch.int64).sum().item() == int(want.astype(np.int64).sum())
    gst.close()


def test_refusals_leave_everything_unqueued(hip):
    import torch
    from theora_amd import _lib
    L = _lib.load()
    a, b = _state(hip, 176, 144, 0, 1), _state(hip, 64, 48, 0, 2)
    fresh = hip.State(64, 48)   # nothing decoded yet
    d = [torch.full((3, 80, 96), 7, dtype=torch.uint8, device="cuda"), torch.full((3, 30, 40), 7, dtype=torch.uint8, device="cuda")]
    i64 = C.c_int64 * 3

    def req(st, out, **kw):
        r = _lib.PictureResizeReq()
        r.state = st.handle if st is not None else None
        r.bufi = -1
        r.format, r.filter, r.elem = _lib.PIC_RGB_PLANAR, _lib.FILTER_AREA, _lib.ELEM_U8
        r.out_width, r.out_height = (out.shape[2], out.shape[1]) if out is not None else (40, 30)
        for p in range(3):
            r.dst[p] = out[p].data_ptr() if out is not None else None
            r.dst_pitch[p] = out.stride(1) if out is not None else 0
            r.scale[p], r.bias[p] = 1.0, 0.0
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    bad = [(_lib.EINVAL, req(b, d[1], x=1, y=0, width=64, height=48)),   # outside the frame
           (_lib.EINVAL, req(b, d[1], width=0, height=5)),
           (_lib.EINVAL, req(b, d[1], format=9)),
           (_lib.EINVAL, req(b, d[1], filter=2)), (_lib.EINVAL, req(b, d[1], filter=-1)),
           (_lib.EINVAL, req(b, d[1], elem=3)), (_lib.EINVAL, req(b, d[1], elem=-1)),
           (_lib.EINVAL, req(b, d[1], format=_lib.PIC_YCBCR, elem=_lib.ELEM_F32, dst_pitch=i64(400, 400, 400))),   # float, not planar
           (_lib.EINVAL, req(b, d[1], format=_lib.PIC_RGBA32, elem=_lib.ELEM_F16, dst_pitch=i64(400, 400, 400))),
           (_lib.EINVAL, req(b, d[1], out_width=0)), (_lib.EINVAL, req(b, d[1], out_height=0)),
           (_lib.EINVAL, req(b, d[1], out_width=16385, dst_pitch=i64(20000, 20000, 20000))),
           (_lib.EINVAL, req(b, d[1], out_height=16385)),
           (_lib.EINVAL, req(b, d[1], bufi=3)),
           (_lib.EINVAL, req(b, d[1], dst_pitch=i64(40, 39, 40))),        # a pitch below the row
           (_lib.EINVAL, req(b, d[1], elem=_lib.ELEM_F16, dst_pitch=i64(80, 80, 79))),      # ... in bytes: 2 a sample
           (_lib.EINVAL, req(b, d[1], elem=_lib.ELEM_F32, dst_pitch=i64(159, 160, 160))),   # ... 4 a sample
           (_lib.EINVAL, req(b, d[1], format=_lib.PIC_RGB24, dst_pitch=i64(119, 0, 0))),
           (_lib.EINVAL, req(b, d[1], format=_lib.PIC_RGBA32, dst_pitch=i64(159, 0, 0))),
           (_lib.EINVAL, req(b, d[1], out_width=1)),                      # area: 64 source columns > 32 x 1
           (_lib.EINVAL, req(b, d[1], out_height=1)),                     # 48 rows > 32 x 1
           # luma 64 rows to 2 is within the limit; the chroma rectangle of rows 1 .. 64 has 33 rows, for one output row
           (_lib.EINVAL, req(a, d[1], format=_lib.PIC_YCBCR, x=0, y=1, width=64, height=64, out_height=2)),
           (_lib.EINVAL, req(fresh, d[1])),
           (_lib.EFAULT, req(b, None)),
           (_lib.EFAULT, req(b, d[1], dst=(C.c_void_p * 3)(d[1][0].data_ptr(), d[1][1].data_ptr(), None))),
           (_lib.EFAULT, req(None, d[1]))]
    for want, r in bad:
        reqs = (_lib.PictureResizeReq * 3)(req(a, d[0]), r, req(a, d[0], filter=_lib.FILTER_BILINEAR))
        assert L.thip_picture_resize(reqs, 3, None) == want
        assert L.thip_picture_resize(C.byref(r), 1, None) == want
        torch.cuda.synchronize()
        hip.synchronize()
        assert (d[0] == 7).all().item() and (d[1] == 7).all().item()
    # bilinear has no such limit, and the limit itself is met exactly at 32
    ok = [req(b, d[1], out_width=1, filter=_lib.FILTER_BILINEAR), req(b, d[1], out_width=2), req(b, d[1], x=0, y=0, width=64, height=32, out_height=1)]
    for r in ok:
        assert L.thip_picture_resize(C.byref(r), 1, None) == 0
    reqs = (_lib.PictureResizeReq * 2)(req(a, d[0]), req(b, d[1]))
    assert L.thip_picture_resize(reqs, 0, None) == 0
    assert L.thip_picture_resize(reqs, 2, None) == 0
    hip.synchronize()
    assert np.array_equal(d[0].cpu().numpy(), _want(a.ycbcr_out(), 0, (96, 80), "rgb_planar", "area"))
    assert np.array_equal(d[1].cpu().numpy(), _want(b.ycbcr_out(), 0, (40, 30), "rgb_planar", "area"))
    for s in (a, b, fresh):
        s.close()


# ---- th_decode_* ----------------------------------------------------------------------------------------------------------
def _check_dec(dec, pf):
    import torch
    planes = dec.ycbcr_out()
    i = dec.info
    crop = (i.pic_x, i.pic_y, i.pic_width, i.pic_height)
    for size, fmt, filt, rect, dtype in (((96, 80), "ycbcr", "area", None, torch.uint8), ((33, 17), "rgb", "bilinear", crop, torch.uint8),
                                         ((64, 64), "rgb_planar", "area", crop, torch.float16)):
        got = _host(dec.picture_resized(size, fmt, filt, rect, dtype=dtype, scale=SCALE, bias=BIAS))
        assert _same(got, _want(planes, pf, size, fmt, filt, rect, dtype)), (size, fmt, filt)


@pytest.mark.parametrize("w,h,pf", [(176, 144, 0), (96, 64, 2), (64, 48, 3)])
def test_decoder_picture_resized(hip, w, h, pf):
    from theora_amd.decoder import Decoder
    st = streamgen.Stream(w, h, pf, 31 + w + pf)
    dec = Decoder(st.header_packets())
    dec.set_host_output(False)
    for f in range(4):
        pkt, _ = st.frame(0 if f == 0 else 1, density=[0.9, 0.5, 0.15][f % 3])
        dec.packetin(pkt)
        _check_dec(dec, pf)
        if f == 2:
            rc, _ = dec.packetin(b"")   # a dropped frame: TH_DUPFRAME, the same picture
            assert rc == 1
            _check_dec(dec, pf)
    dec.close()


def test_decoder_picture_resized_before_the_first_frame(hip):
    from theora_amd import _lib
    from theora_amd.decoder import Decoder, PictureResizeArgs, TH_DECCTL_THIP_PICTURE_RESIZE
    st = streamgen.Stream(64, 48, 0, 3)
    dec = Decoder(st.header_packets())
    a = PictureResizeArgs()
    assert dec.ctl(TH_DECCTL_THIP_PICTURE_RESIZE, a, C.sizeof(a)) == _lib.EINVAL
    assert dec.ctl(TH_DECCTL_THIP_PICTURE_RESIZE, a, C.sizeof(a) - 4) == _lib.EINVAL
    assert dec.ctl(TH_DECCTL_THIP_PICTURE_RESIZE, None, 0) == _lib.EFAULT
    dec.close()


def test_transcoding_to_a_smaller_size(hip):
    """decode -> resize -> TH_ENCCTL_THIP_YCBCR_IN_DEVICE on one stream, nothing waited for in between: the packets are those of an
    encoder given the restatement's planes through th_encode_ycbcr_in."""
    import torch
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    w, h, size = 176, 144, (96, 80)
    src = streamgen.Stream(w, h, 0, 404)
    pkts = [src.frame(0 if f == 0 else 1, density=[0.9, 0.5, 0.3][f % 3])[0] for f in range(5)]
    dec = Decoder(src.header_packets())
    cfg = dict(quality=40, inter=True)
    dev_enc, ref_enc = Encoder(size[0], size[1], 0, **cfg), Encoder(size[0], size[1], 0, **cfg)
    assert dev_enc.header_packets() == ref_enc.header_packets()
    s = torch.cuda.Stream()
    got, want, kinds = [], [], []
    for f, pkt in enumerate(pkts):
        dec.packetin(pkt)
        planes = dec.picture_resized(size, "ycbcr", "area", stream=s)
        dev_enc.encode(planes, stream=s)
        ref_enc.encode(rr.resize(dec.ycbcr_out(), 0, size, "ycbcr", "area"))
        for e, out in ((dev_enc, got), (ref_enc, want)):
            while True:
                r = e.packetout(f == len(pkts) - 1)
                if r is None:
                    break
                out.append(r)
        kinds.append(got[-1][0][0] & 0x40)
    assert len(got) == len(pkts) and got == want
    assert kinds[0] == 0 and any(kinds[1:])          # a key frame, then inter frames
    for x in (dec, dev_enc, ref_enc):
        x.close()
