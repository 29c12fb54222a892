"""R'G'B' picture input on the GPU (thip_picture_in / k_picture_in, TH_ENCCTL_THIP_RGB_IN): the planes equal the numpy restatement
(tests/picture_in_ref.py) byte for byte, whatever the alignment and pitch of source and destination, and read or write nothing
around them; batching and stream order hold; the encoder's packets from R'G'B' equal the packets of the restatement's planes in
every mode."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import picture_in_ref

pytestmark = pytest.mark.gpu

FORMATS = ["rgb", "rgba", "rgb_planar"]
CANARY = 0xA5
GUARD = 64


def _image(w, h, seed):
    """Seeded noise over a gradient, (h, w, 3) uint8 -- no pixel equals the canary in all components for long."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * x + y) % 256, (x + 5 * y + 60) % 256, (255 - 2 * x + 3 * y) % 256], -1)
    return ((base + rng.integers(-40, 41, (h, w, 3))) % 256).astype(np.uint8)


def _as_format(img, fmt, seed=0):
    if fmt == "rgb":
        return img
    if fmt == "rgba":
        a = np.random.default_rng(seed + 1).integers(0, 256, img.shape[:2] + (1,), dtype=np.uint8)   # A is never used
        return np.concatenate([img, a], 2)
    return np.ascontiguousarray(img.transpose(2, 0, 1))


@functools.lru_cache(maxsize=None)
def _case(w, h, px, py, fmt, pf):
    """(source array in its format, the restatement's planes): computed once, shared, never written."""
    src = _as_format(_image(w, h, 1000 * w + h + px), fmt, w)
    want = picture_in_ref.picture_in(src, pf, fmt, px, py)
    src.setflags(write=False)
    for p in want:
        p.setflags(write=False)
    return src, want


def _embed(arr, pad, off):
    """A 2-D (rows, row bytes) uint8 array as a view inside a larger device buffer full of the canary: row pitch = row bytes
    + pad, the first byte GUARD + off bytes into the allocation.  Returns (buffer, view of shape (rows, row bytes))."""
    import torch
    rows, rb = arr.shape
    pitch = rb + pad
    host = np.full(2 * GUARD + off + rows * pitch, CANARY, np.uint8)
    body = host[GUARD + off:GUARD + off + rows * pitch].reshape(rows, pitch)
    body[:, :rb] = arr
    buf = torch.from_numpy(host).cuda()
    return buf, torch.as_strided(buf, (rows, rb), (pitch, 1), GUARD + off)


def _source(src, fmt, pad, off):
    """The picture as device views with the given padding and offset; (views for picture_in, buffers to keep)."""
    import torch
    if fmt == "rgb_planar":
        pairs = [_embed(src[c], pad, off) for c in range(3)]
        return [v for _, v in pairs], [b for b, _ in pairs]
    h, w, c = src.shape
    buf, v = _embed(src.reshape(h, w * c), pad, off)
    return torch.as_strided(buf, (h, w, c), (v.stride(0), c, 1), v.storage_offset()), [buf]


def _check_dest(bufs, views, want, pad, off, what):
    for (buf, v, wp) in zip(bufs, views, want):
        rows, rb = wp.shape
        pitch = rb + pad
        b = buf.cpu().numpy()
        body = b[GUARD + off:GUARD + off + rows * pitch].reshape(rows, pitch)
        assert np.array_equal(body[:, :rb], wp), what
        assert (body[:, rb:] == CANARY).all(), what                      # the rows' padding
        assert (b[:GUARD + off] == CANARY).all() and (b[GUARD + off + rows * pitch:] == CANARY).all(), what


def _run_case(hip, w, h, px, py, fmt, pf, variants):
    import torch
    src, want = _case(w, h, px, py, fmt, pf)
    for pad, off in variants:
        s_views, keep = _source(src, fmt, pad, off)
        dst = [_embed(np.full(p.shape, CANARY, np.uint8), pad, off) for p in want]
        out = hip.picture_in([s_views], pf, fmt, pics=[(px, py)], outs=[[v for _, v in dst]])
        torch.cuda.synchronize()
        assert [tuple(o.shape) for o in out[0]] == picture_in_ref.plane_shapes(w, h, pf, px, py)
        _check_dest([b for b, _ in dst], [v for _, v in dst], want, pad, off, (w, h, px, py, fmt, pf, pad, off))
        del keep


VARIANTS = [(0, 0), (5, 0), (0, 1), (5, 1)]   # (bytes of padding a row, offset of the base): tight / padded, 16-byte path or not
PICTURES = [(1, 1, 0, 0), (2, 2, 1, 1), (17, 9, 3, 5), (33, 18, 0, 1), (176, 144, 0, 0)]


@pytest.mark.parametrize("pf", [0, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h,px,py", PICTURES)
def test_planes_equal_the_restatement(hip, w, h, px, py, fmt, pf):
    _run_case(hip, w, h, px, py, fmt, pf, VARIANTS)


@pytest.mark.parametrize("fmt", FORMATS)
def test_planes_equal_the_restatement_1080p(hip, fmt):
    _run_case(hip, 1920, 1080, 0, 4, fmt, 0, VARIANTS)


def test_made_destinations_and_odd_offsets_at_every_subsampling(hip):
    """outs=None: the call makes the planes; odd pic_x with widths around the 16-pixel chunk, odd pic_y with odd heights."""
    import torch
    for pf in (0, 2, 3):
        for (w, h, px, py) in [(16, 15, 1, 1), (15, 2, 1, 0), (32, 3, 1, 1), (31, 16, 3, 2), (48, 5, 0, 1)]:
            img = _image(w, h, w + h)
            src = torch.from_numpy(img).cuda()
            got = hip.picture_in([src], pf, "rgb", pics=[(px, py)])[0]
            torch.cuda.synchronize()
            want = picture_in_ref.picture_in(img, pf, "rgb", px, py)
            for p in range(3):
                assert np.array_equal(got[p].cpu().numpy(), want[p]), (pf, w, h, px, py, p)


def test_batch_of_nine_is_chunked(hip):
    import torch
    cases = [(176, 144, 0, 0, "rgb", 0), (17, 9, 3, 5, "rgba", 2), (33, 18, 0, 1, "rgb_planar", 3), (64, 48, 1, 1, "rgb", 3),
             (1, 1, 0, 0, "rgba", 0), (100, 31, 1, 0, "rgb_planar", 0), (31, 100, 0, 1, "rgb", 2), (320, 240, 2, 2, "rgba", 0),
             (2, 2, 1, 1, "rgb_planar", 2)]
    srcs = []
    for (w, h, px, py, fmt, pf) in cases:
        a = _as_format(_image(w, h, w * h + pf), fmt, w)
        srcs.append((a, torch.from_numpy(np.array(a)).cuda()))
    single = [[p.cpu().numpy() for p in hip.picture_in([t], pf, fmt, pics=[(px, py)])[0]]
              for (a, t), (w, h, px, py, fmt, pf) in zip(srcs, cases)]
    outs = hip.picture_in([t for _, t in srcs], [c[5] for c in cases], [c[4] for c in cases], pics=[(c[2], c[3]) for c in cases])
    torch.cuda.synchronize()
    for k, ((a, t), (w, h, px, py, fmt, pf)) in enumerate(zip(srcs, cases)):
        want = picture_in_ref.picture_in(a, pf, fmt, px, py)
        for p in range(3):
            assert np.array_equal(outs[k][p].cpu().numpy(), single[k][p]), (k, p)
            assert np.array_equal(single[k][p], want[p]), (k, p)


def test_ordering_on_a_torch_stream(hip):
    """Fill the source, call, overwrite the source on the same stream: the result is the first content's."""
    import torch
    w, h = 320, 240
    first, second = _image(w, h, 1), _image(w, h, 2)
    want = picture_in_ref.picture_in(first, 0, "rgb")
    a, b = torch.from_numpy(first).cuda(), torch.from_numpy(second).cuda()
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    big = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):            # keep the stream busy: the conversion starts late
            big.add_(1)
        src.copy_(a)
        out = hip.picture_in([src], 0, "rgb", stream=s)[0]
        src.copy_(b)
        after = [p.clone() for p in out]
    torch.cuda.synchronize()
    for p in range(3):
        assert np.array_equal(out[p].cpu().numpy(), want[p]), p
        assert np.array_equal(after[p].cpu().numpy(), want[p]), p
    # torch's default (null) stream
    src.copy_(b)
    out = hip.picture_in([src], 0, "rgb")[0]
    total = sum(int(p.to(torch.int64).sum().item()) for p in out)
    assert total == sum(int(p.astype(np.int64).sum()) for p in picture_in_ref.picture_in(second, 0, "rgb"))


def test_all_or_nothing(hip):
    import torch
    from theora_amd import _lib
    L = _lib.load()
    img = torch.from_numpy(_image(32, 16, 3)).cuda()
    dst = [torch.full(sh, 7, dtype=torch.uint8, device="cuda") for sh in picture_in_ref.plane_shapes(32, 16, 0)]

    def req(**kw):
        r = _lib.PictureInReq()
        r.format, r.pixel_fmt, r.width, r.height = _lib.PIC_RGB24, 0, 32, 16
        r.src[0], r.src_pitch[0] = img.data_ptr(), img.stride(0)
        for p in range(3):
            r.dst[p], r.dst_pitch[p] = dst[p].data_ptr(), dst[p].stride(0)
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    for want, r in [(_lib.EINVAL, req(format=_lib.PIC_YCBCR)), (_lib.EINVAL, req(src_pitch=(C.c_int64 * 3)(95, 0, 0))),
                    (_lib.EFAULT, req(dst=(C.c_void_p * 3)(dst[0].data_ptr(), None, dst[2].data_ptr())))]:
        reqs = (_lib.PictureInReq * 2)(req(), r)
        assert L.thip_picture_in(reqs, 2, None) == want
        torch.cuda.synchronize()
        assert all((d == 7).all().item() for d in dst)
    assert L.thip_picture_in(req(), 1, None) == 0
    torch.cuda.synchronize()
    want = picture_in_ref.picture_in(img.cpu().numpy(), 0, "rgb")
    assert all(np.array_equal(d.cpu().numpy(), p) for d, p in zip(dst, want))


# ---- th_encode_* ----------------------------------------------------------------------------------------------------------------
W, H, PIC = 64, 48, (1, 2, 61, 45)
CONFIGS = {
    "intra_q63": dict(quality=63),
    "modes_bqi_pack": dict(quality=40, inter=True, all_modes=True, block_qi=8, device_pack=True),
    "bitrate_inter": dict(quality=32, inter=True, bitrate=60000),
    "auto_keyframes": dict(quality=40, inter=True, auto_keyframes=True),
}


@functools.lru_cache(maxsize=None)
def _frames(cut):
    """Four R'G'B' pictures, seeded noise over a gradient that moves; with cut, the content changes at frame 2."""
    out = []
    for f in range(4):
        rng = np.random.default_rng(50 + f)
        y, x = np.mgrid[0:PIC[3], 0:PIC[2]]
        x = x + 2 * f
        base = np.stack([(4 * x + y) % 256, (x + 3 * y + 60) % 256, (255 - 2 * x + y) % 256], -1)
        if cut and f >= 2:
            base = np.stack([(7 * y + 90) % 256, (200 - 5 * x) % 256, (x * y) % 256], -1)
        img = np.clip(base + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8)
        img.setflags(write=False)
        out.append(img)
    return out


def _packets(e, feed, frames):
    out = []
    for f, fr in enumerate(frames):
        feed(e, fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def _reference_packets(name, pf):
    """The packets of an Encoder fed the restatement's planes through encode(): (headers, packets)."""
    from theora_amd.encoder import Encoder
    frames = _frames(name == "auto_keyframes")
    e = Encoder(W, H, pf, pic=PIC, **CONFIGS[name])
    hdr = e.header_packets()
    out = _packets(e, lambda e, fr: e.encode(picture_in_ref.picture_in(fr, pf, "rgb", PIC[0], PIC[1])), frames)
    e.close()
    assert len(out) == len(frames)
    return hdr, out


def _feed_rgb(path, fmt):
    import torch

    def feed(e, fr):
        a = _as_format(fr, fmt, 5)
        if path == "device":
            e.encode_rgb(torch.from_numpy(np.array(a)).cuda(), fmt)
        elif path == "device_pitch":      # rows with a pitch of their own inside a larger tensor
            if fmt == "rgb_planar":
                big = torch.full((3, a.shape[1], a.shape[2] + 7), CANARY, dtype=torch.uint8, device="cuda")
                big[:, :, :a.shape[2]] = torch.from_numpy(np.array(a)).cuda()
                e.encode_rgb([big[c, :, :a.shape[2]] for c in range(3)], fmt)
            else:
                big = torch.full((a.shape[0], a.shape[1] + 3, a.shape[2]), CANARY, dtype=torch.uint8, device="cuda")
                big[:, :a.shape[1]] = torch.from_numpy(np.array(a)).cuda()
                e.encode_rgb(big[:, :a.shape[1]], fmt)
        elif path == "host":
            e.encode_rgb(a, fmt)
        else:                             # host rows with a pitch of their own
            if fmt == "rgb_planar":
                big = np.full((3, a.shape[1], a.shape[2] + 7), CANARY, np.uint8)
                big[:, :, :a.shape[2]] = a
                e.encode_rgb(big[:, :, :a.shape[2]], fmt)
            else:
                big = np.full((a.shape[0], a.shape[1] + 3, a.shape[2]), CANARY, np.uint8)
                big[:, :a.shape[1]] = a
                e.encode_rgb(big[:, :a.shape[1]], fmt)
    return feed


@pytest.mark.parametrize("pf", [0, 3])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_encoder_packets_equal_those_of_the_restatements_planes(hip, name, pf):
    from theora_amd.encoder import Encoder
    frames = _frames(name == "auto_keyframes")
    hdr, want = _reference_packets(name, pf)
    for path, fmt in [("device", "rgb"), ("host", "rgb"), ("device_pitch", "rgba"), ("host_pitch", "rgb_planar"), ("device", "rgb_planar"),
                      ("host", "rgba")]:
        e = Encoder(W, H, pf, pic=PIC, **CONFIGS[name])
        assert e.header_packets() == hdr
        got = _packets(e, _feed_rgb(path, fmt), frames)
        e.close()
        assert len(got) == len(want), (path, fmt)
        for f, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, (path, fmt, f)


def test_auto_keyframes_cut_where_the_content_changes(hip):
    """The configuration above really exercises the measurement: frame 2 is measured and cut, frames 1 and 3 measured and kept."""
    from theora_amd.encoder import Encoder
    e = Encoder(W, H, 0, pic=PIC, **CONFIGS["auto_keyframes"])
    e.header_packets()
    stats = []
    for f, fr in enumerate(_frames(True)):
        e.encode_rgb(fr)
        assert e.packetout(f == 3) is not None
        stats.append(e.cut_stats())
    e.close()
    assert [s["measured"] for s in stats] == [0, 1, 1, 1] and [s["cut"] for s in stats] == [0, 0, 1, 0]


def test_packets_decode_to_the_encoders_reconstruction(hip):
    """End to end: R'G'B' in, packets out, through this library's decoder -- and the reference decoder where it is built -- to the
    encoder's own reconstruction."""
    from oracle import ref
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    import torch
    e = Encoder(W, H, 0, pic=PIC, **CONFIGS["modes_bqi_pack"])
    hdr = e.header_packets()
    dec = Decoder(hdr)
    rd = ref.RefDecoder(hdr) if ref.available() else None
    for f, fr in enumerate(_frames(False)):
        e.encode_rgb(torch.from_numpy(np.array(fr)).cuda())
        pkt = e.packetout(f == 3)
        assert pkt is not None
        want = e.recon()
        assert dec.packetin(pkt[0])[0] == 0
        got = dec.ycbcr_out()
        for p in range(3):
            assert np.array_equal(got[p], want[p]), (f, p)
        if rd is not None:
            assert rd.packetin(pkt[0])[0] == 0
            got = rd.ycbcr_out()
            for p in range(3):
                assert np.array_equal(got[p], want[p]), ("reference", f, p)
    # the reconstruction is the picture that went in, to the quantiser's accuracy
    y = picture_in_ref.picture_in(_frames(False)[3], 0, "rgb", PIC[0], PIC[1])[0].astype(np.int64)
    err = want[0][PIC[1]:PIC[1] + PIC[3], PIC[0]:PIC[0] + PIC[2]].astype(np.int64) - y
    assert np.abs(err).mean() < 8
    dec.close()
    if rd is not None:
        rd.close()
    e.close()


def test_tensor_may_be_overwritten_straight_after_encode_rgb(hip):
    import torch
    from theora_amd.encoder import Encoder
    frames = _frames(False)
    hdr, want = _reference_packets("modes_bqi_pack", 0)
    e = Encoder(W, H, 0, pic=PIC, **CONFIGS["modes_bqi_pack"])
    e.header_packets()
    s = torch.cuda.Stream()
    t = torch.zeros((PIC[3], PIC[2], 3), dtype=torch.uint8, device="cuda")
    dev = [torch.from_numpy(np.array(fr)).cuda() for fr in frames]
    big = torch.zeros(16 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = []
    for f in range(4):
        with torch.cuda.stream(s):
            big.add_(1)               # the conversion starts late
            t.copy_(dev[f])
            e.encode_rgb(t, stream=s)
            t.fill_(CANARY)           # at once, on the caller's stream
        got.append(e.packetout(f == 3))
    torch.cuda.synchronize()
    e.close()
    assert got == want


def test_encode_rgb_with_a_frame_pending(hip):
    from theora_amd import _lib
    from theora_amd.encoder import TH_ENCCTL_THIP_RGB_IN, Encoder, RgbIn, RGB_FORMATS
    frames = _frames(False)
    hdr, want = _reference_packets("intra_q63", 0)
    e = Encoder(W, H, 0, pic=PIC, **CONFIGS["intra_q63"])
    e.header_packets()
    e.encode_rgb(frames[0])
    other = np.ascontiguousarray(frames[1])
    a = RgbIn()
    a.format, a.device, a.width, a.height = RGB_FORMATS["rgb"], 0, PIC[2], PIC[3]
    a.src[0], a.pitch[0] = other.ctypes.data, other.strides[0]
    assert e._L.th_encode_ctl(e._enc, TH_ENCCTL_THIP_RGB_IN, C.byref(a), C.sizeof(a)) == _lib.EINVAL
    with pytest.raises(_lib.TheoraHipError):
        e.encode_rgb(frames[1])
    assert e.packetout(False) == want[0]            # the pending frame's packet is intact
    e.encode_rgb(frames[1])
    assert e.packetout(False) == want[1]
    e.encode_rgb(frames[2])
    assert e.packetout(True)[:3] == want[2][:3]
    assert e._L.th_encode_ctl(e._enc, TH_ENCCTL_THIP_RGB_IN, C.byref(a), C.sizeof(a)) == _lib.EINVAL   # after the last packet
    e.close()
