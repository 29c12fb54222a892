"""Pictures that stay on the device (thip_picture_out / TH_DECCTL_THIP_PICTURE_OUT, k_picture_out): bit-exact against the numpy
restatement of the definitions (tests/picture_ref.py) applied to State.ycbcr_out() / Decoder.ycbcr_out(), which the other GPU
tests check against the oracle; plus ordering, alignment and all-or-nothing checks."""
import ctypes as C

import numpy as np
import pytest

from tests import picture_ref, streamgen

pytestmark = pytest.mark.gpu

FORMATS = [("ycbcr", "linear"), ("rgb", "nearest"), ("rgb", "linear"), ("rgba", "nearest"), ("rgba", "linear"),
           ("rgb_planar", "nearest"), ("rgb_planar", "linear")]


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


def _same(got, want):
    if isinstance(want, list):
        return all(np.array_equal(g, w) for g, w in zip(got, want))
    return np.array_equal(got, want)


@pytest.mark.parametrize("fmt", [0, 2, 3])
@pytest.mark.parametrize("w,h", [(16, 16), (176, 144), (1280, 720), (1920, 1088)])
def test_every_format_and_rectangle(hip, w, h, fmt):
    import torch
    st = _state(hip, w, h, fmt, w + h + fmt)
    planes = st.ycbcr_out()
    rects = [None] + [r for r in [(0, 0, 1920, 1080), (3, 5, 101, 77)] if r[0] + r[2] <= w and r[1] + r[3] <= h]
    for rect in rects:
        for f, ch in FORMATS:
            got = _host(st.picture(f, ch, rect))
            torch.cuda.synchronize()
            assert _same(got, picture_ref.picture(planes, fmt, f, ch, rect)), (rect, f, ch)
    st.close()


def test_postprocessed_and_as_decoded(hip):
    from theora_amd import _lib
    L = _lib.load()
    w, h, fmt = 176, 144, 0
    st = _state(hip, w, h, fmt, 7)
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
    for f, ch in FORMATS:
        assert _same(_host(st.picture(f, ch)), picture_ref.picture(pp, fmt, f, ch)), (f, ch)
        assert _same(_host(st.picture(f, ch, bufi=0)), picture_ref.picture(decoded, fmt, f, ch)), (f, ch)
    st.close()


def test_batch_of_nine_is_chunked(hip):
    import theora_amd
    import torch
    sizes = [(176, 144, 0), (64, 48, 2), (48, 80, 3), (320, 240, 0), (16, 16, 0), (176, 144, 3), (128, 64, 2), (96, 96, 0),
             (1280, 720, 0)]
    states = [_state(hip, w, h, f, 100 + i) for i, (w, h, f) in enumerate(sizes)]
    fmts = [FORMATS[i % len(FORMATS)] for i in range(len(states))]
    rects = [None if i % 2 else (3, 5, 11, 9) for i in range(len(states))]
    single = [_host(s.picture(f, c, r)) for s, (f, c), r in zip(states, fmts, rects)]
    outs = []
    for s, (f, c), r in zip(states, fmts, rects):
        x, y, w, h = r if r else (0, 0, s.frame_width, s.frame_height)
        shp = theora_amd.picture_shapes(f, w, h, x, s.pixel_fmt, y)
        outs.append([torch.zeros(p, dtype=torch.uint8, device="cuda") for p in shp] if f == "ycbcr"
                    else torch.zeros(shp, dtype=torch.uint8, device="cuda"))
    theora_amd.picture_out(states, outs, [f for f, _ in fmts], [c for _, c in fmts], rects)
    for k, (o, want) in enumerate(zip(outs, single)):
        assert _same(_host(o), want), k
    for s in states:
        s.close()


def _decode(hip, gst, geom, rng, ftype, keep):
    from theora_amd import synth
    fr = synth.gen_frame(geom, rng, ftype, "mixed", flimit=4)
    desc, ka = synth.upload_frame(synth.pack_frame(geom, fr))
    keep.append(ka)
    hip.decode_frames([gst], [desc])


def test_ordering_on_a_torch_stream(hip):
    import torch
    from theora_amd import synth
    w, h = 176, 144
    geom = synth.Geometry(w, h)
    rng = np.random.default_rng(11)
    gst = hip.State(w, h)
    keep = []
    _decode(hip, gst, geom, rng, hip.INTRA_FRAME, keep)
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)
    want = picture_ref.picture(gst.ycbcr_out(), 0, "rgba", "linear")
    s = torch.cuda.Stream()
    big = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(8):           # keep the stream busy: the picture starts late
            big.add_(1)
        out = gst.picture("rgba", "linear", stream=s)
        after = out.clone()          # a torch op behind the call on the same stream
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)   # the second of these writes the buffer the picture reads
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)
    torch.cuda.synchronize()
    hip.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(after.cpu().numpy(), want)
    # torch's default (null) stream
    want = picture_ref.picture(gst.ycbcr_out(), 0, "rgb", "nearest")
    out = gst.picture("rgb", "nearest")
    total = out.to(torch.int64).sum().item()
    assert total == int(want.astype(np.int64).sum())
    gst.close()


@pytest.mark.parametrize("rect", [None, (3, 5, 101, 77)])
def test_unaligned_destinations_and_guard_bytes(hip, rect):
    import theora_amd
    import torch
    w, h, fmt = 176, 144, 0
    st = _state(hip, w, h, fmt, 5)
    planes = st.ycbcr_out()
    x, y, rw, rh = rect if rect else (0, 0, w, h)
    for f, ch in FORMATS:
        want = picture_ref.picture(planes, fmt, f, ch, rect)
        shp = theora_amd.picture_shapes(f, rw, rh, x, fmt, y)
        pshapes = shp if f == "ycbcr" else ([shp[1:]] * 3 if f == "rgb_planar" else [shp])
        bufs, views = [], []
        for ps in pshapes:
            rowbytes = int(np.prod(ps[1:]))
            pitch = rowbytes + (1 if rowbytes % 2 == 0 else 2)   # odd
            guard = 64
            buf = torch.full((2 * guard + 1 + ps[0] * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
            strides = (pitch,) + ((ps[2], 1) if len(ps) == 3 else (1,))
            views.append(torch.as_strided(buf, ps, strides, guard + 1))
            bufs.append((buf, pitch, rowbytes, guard))
        out = views if f in ("ycbcr", "rgb_planar") else views[0]
        theora_amd.picture_out([st], [out], f, ch, [rect])
        torch.cuda.synchronize()
        wl = want if f == "ycbcr" else (list(want) if f == "rgb_planar" else [want])
        for (buf, pitch, rowbytes, guard), wp in zip(bufs, wl):
            b = buf.cpu().numpy()
            body = b[guard + 1:guard + 1 + wp.shape[0] * pitch].reshape(wp.shape[0], pitch)
            assert np.array_equal(body[:, :rowbytes].reshape(wp.shape), wp), (f, ch)
            assert (body[:, rowbytes:] == 0xA5).all(), (f, ch)
            assert (b[:guard + 1] == 0xA5).all() and (b[guard + 1 + wp.shape[0] * pitch:] == 0xA5).all(), (f, ch)
    st.close()


def test_all_or_nothing(hip):
    import torch
    from theora_amd import _lib
    L = _lib.load()
    a, b = _state(hip, 176, 144, 0, 1), _state(hip, 64, 48, 0, 2)
    fresh = hip.State(64, 48)   # nothing decoded yet
    d = [torch.full((144, 176, 4), 7, dtype=torch.uint8, device="cuda"), torch.full((48, 64, 4), 7, dtype=torch.uint8, device="cuda")]

    def req(st, dst, **kw):
        r = _lib.PictureReq()
        r.state = st.handle if st is not None else None
        r.bufi = -1
        r.format = _lib.PIC_RGBA32
        r.chroma = _lib.CHROMA_LINEAR
        r.dst[0] = dst.data_ptr() if dst is not None else None
        r.dst_pitch[0] = dst.stride(0) if dst is not None else 0
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    bad = [(_lib.EINVAL, req(b, d[1], x=1, y=0, width=64, height=48)),   # outside the frame
           (_lib.EINVAL, req(b, d[1], format=9)),
           (_lib.EINVAL, req(b, d[1], chroma=5)),
           (_lib.EINVAL, req(b, d[1], bufi=3)),
           (_lib.EINVAL, req(b, d[1], dst_pitch=(C.c_int64 * 3)(255, 0, 0))),
           (_lib.EINVAL, req(fresh, d[1])),
           (_lib.EINVAL, req(b, d[1], width=0, height=5)),
           (_lib.EFAULT, req(b, None)),
           (_lib.EFAULT, req(None, d[1]))]
    for want, r in bad:
        reqs = (_lib.PictureReq * 3)(req(a, d[0]), r, req(a, d[0], format=_lib.PIC_RGB24))
        assert L.thip_picture_out(reqs, 3, None) == want
        torch.cuda.synchronize()
        hip.synchronize()
        assert (d[0] == 7).all().item() and (d[1] == 7).all().item()
    reqs = (_lib.PictureReq * 2)(req(a, d[0]), req(b, d[1]))
    assert L.thip_picture_out(reqs, 0, None) == 0
    assert L.thip_picture_out(reqs, 2, None) == 0
    hip.synchronize()
    assert np.array_equal(d[0].cpu().numpy(), picture_ref.picture(a.ycbcr_out(), 0, "rgba", "linear"))
    for s in (a, b, fresh):
        s.close()


# ---- th_decode_* ----------------------------------------------------------------------------------------------------------
PIC = (3, 5)   # th_info's pic_x, pic_y (from the top)


def _headers(st, pw, ph):
    """streamgen's headers with the info header re-packed for a picture region of pw x ph at PIC (the header counts PICY
    from the bottom, th_info from the top)."""
    hdr = st.header_packets()
    bw = streamgen.BitWriter()
    bw.write(0x80, 8)
    for c in b"theora":
        bw.write(c, 8)
    for v, n in ((3, 8), (2, 8), (1, 8), (st.w >> 4, 16), (st.h >> 4, 16), (pw, 24), (ph, 24),
                 (PIC[0], 8), (st.h - ph - PIC[1], 8), (30, 32), (1, 32), (1, 24), (1, 24), (0, 8), (0, 24), (32, 6),
                 (st.kfgshift, 5), (st.fmt, 2), (0, 3)):
        bw.write(v, n)
    return [bw.bytes()] + hdr[1:]


def _check_dec(dec, fmt_px, formats=(("rgb", "linear"), ("ycbcr", "linear"), ("rgba", "nearest"))):
    import torch
    planes = dec.ycbcr_out()
    i = dec.info
    rect = (i.pic_x, i.pic_y, i.pic_width, i.pic_height)
    for f, ch in formats:
        got = _host(dec.picture(f, ch, crop=True))
        torch.cuda.synchronize()
        assert _same(got, picture_ref.picture(planes, fmt_px, f, ch, rect)), (f, ch)
    got = _host(dec.picture("rgb", "linear", crop=False))
    assert np.array_equal(got, picture_ref.picture(planes, fmt_px, "rgb", "linear"))


@pytest.mark.parametrize("host_output", [True, False])
@pytest.mark.parametrize("w,h,fmt", [(176, 144, 0), (96, 64, 2), (64, 48, 3)])
def test_decoder_picture(hip, w, h, fmt, host_output):
    from theora_amd.decoder import Decoder
    st = streamgen.Stream(w, h, fmt, 21 + w + fmt)
    pw, ph = w - 3 - 6, h - 5 - 4
    dec = Decoder(_headers(st, pw, ph))
    assert (dec.info.pic_x, dec.info.pic_y, dec.info.pic_width, dec.info.pic_height) == (PIC[0], PIC[1], pw, ph)
    dec.set_host_output(host_output)
    for f in range(6):
        pkt, truth = st.frame(0 if f % 4 == 0 else 1, density=[0.9, 0.5, 0.15][f % 3])
        dec.packetin(pkt)
        _check_dec(dec, fmt)
        if f == 2:
            rc, _ = dec.packetin(b"")   # a dropped frame: TH_DUPFRAME, the same picture
            assert rc == 1
            _check_dec(dec, fmt)
    dec.close()


def test_decoder_picture_before_the_first_frame(hip):
    from theora_amd import _lib
    from theora_amd.decoder import Decoder, PictureOutArgs, TH_DECCTL_THIP_PICTURE_OUT
    st = streamgen.Stream(64, 48, 0, 3)
    dec = Decoder(st.header_packets())
    a = PictureOutArgs()
    assert dec._L.th_decode_ctl(dec._dec, TH_DECCTL_THIP_PICTURE_OUT, C.byref(a), C.sizeof(a)) == _lib.EINVAL
    dec.close()


def test_decoder_picture_with_packets_announced_ahead(hip):
    from theora_amd.decoder import Decoder
    w, h, fmt = 176, 144, 0
    st = streamgen.Stream(w, h, fmt, 77)
    pkts = [st.frame(0 if f % 5 == 0 else 1, density=[0.9, 0.5, 0.15][f % 3])[0] for f in range(10)]
    dec = Decoder(_headers(st, w - 9, h - 9))
    announced = 0
    for f in range(len(pkts)):
        while announced < len(pkts) and announced < f + 4:   # announced in decode order, the packet at hand included
            dec.prefetch(pkts[announced])
            announced += 1
        dec.packetin(pkts[f])
        _check_dec(dec, fmt)   # ycbcr_out may decode the next packet ahead; the picture is still this frame's
    dec.close()


def test_decoder_picture_after_a_take_back(hip):
    from theora_amd.decoder import Decoder
    w, h, fmt = 176, 144, 0
    st = streamgen.Stream(w, h, fmt, 78)
    pkts = [st.frame(0 if f == 0 else 1, density=0.5)[0] for f in range(4)]
    other = st.frame(0, density=0.9)[0]     # a key frame: decodable after any picture
    hdr = _headers(st, w - 9, h - 9)
    ref = Decoder(hdr)
    dec = Decoder(hdr)
    for f in range(3):
        ref.packetin(pkts[f])
        ref.ycbcr_out()
        dec.packetin(pkts[f])
        if f == 2:
            dec.prefetch(pkts[3])
        dec.ycbcr_out()
    dec.packetin(other)   # not the announced packet: the frame decoded ahead (if any) is taken back
    ref.packetin(other)
    for f, ch in (("rgb", "linear"), ("ycbcr", "linear")):
        assert _same(_host(dec.picture(f, ch)), _host(ref.picture(f, ch))), f
    _check_dec(dec, fmt)
    dec.close()
    ref.close()
