"""Picture metrics on the device (thip_picture_compare / TH_DECCTL_THIP_PICTURE_COMPARE / the encoder's quality statistics,
k_picture_compare): every number exact against the numpy restatement of the definition (tests/picture_compare_ref.py) applied to
State.ycbcr_out() / Decoder.ycbcr_out(), which the other GPU tests check against the oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import picture_compare_ref as cr, streamgen

pytestmark = pytest.mark.gpu

BOTH = cr.SSE | cr.SSIM
EXTENTS = [(1, 1), (7, 9), (8, 8), (9, 7), (12, 13), (13, 12), (16, 17), (17, 16), (63, 65), (64, 64), (65, 63)]


def _state(hip, w, h, fmt, seed, fill=None):
    """A state whose newest frame is random content (or the value `fill`) written into buffer 0."""
    st = hip.State(w, h, fmt)
    rng = np.random.default_rng(seed)
    for pli in range(3):
        g = st.planes[pli]
        a = rng.integers(0, 256, (g["height"], g["width"]), dtype=np.uint8) if fill is None else np.full((g["height"], g["width"]), fill, np.uint8)
        st.write_plane(0, pli, a)
    st.set_ref_idx(0, 0, 0)
    return st


def _other(src, seed):
    """The other picture for the rectangles `src`: near the source in the left half (SSIM close to 1), unrelated in the right."""
    rng = np.random.default_rng(seed)
    out = []
    for s in src:
        near = np.clip(s.astype(np.int64) + rng.integers(-6, 7, s.shape), 0, 255).astype(np.uint8)
        far = rng.integers(0, 256, s.shape, dtype=np.uint8)
        out.append(np.where(np.arange(s.shape[1])[None, :] < (s.shape[1] + 1) // 2, near, far).astype(np.uint8))
    return out


def _device(planes, off=0, pad=0):
    """The planes on the device, each starting `off` bytes past an allocation's start at a pitch of width + pad: off = 0 with a
    pitch that is a multiple of 16 lets whole 16-byte loads happen, an odd off or pitch rules them out."""
    import torch
    out = []
    for a in planes:
        h, w = a.shape
        flat = torch.full((off + h * (w + pad) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        v = flat[off:off + h * (w + pad)].view(h, w + pad)[:, :w]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
        out.append(v)
    return out


def _rec(t):
    return [int(v) for v in t.cpu().tolist()]


def _check(st, rect, flags, seed, off=0, pad=0, bufi=-1, planes=None):
    planes = st.ycbcr_out() if planes is None else planes
    src = cr.source_planes(planes, st.pixel_fmt, rect)
    ref = _other(src, seed)
    res, blk = st.compare(_device(ref, off, pad), flags, rect, bufi, blocks=True)
    assert _rec(res) == cr.compare_planes(src, ref, flags), (rect, flags, off, pad)
    want = [cr.block_sse(s, r) for s, r in zip(src, ref)]
    for p in range(3):
        got = blk[p].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert np.array_equal(got, want[p]), (rect, p)
        if flags & cr.SSE:
            assert int(got.sum()) == _rec(res)[p]            # the blocks add up to the plane


@pytest.mark.parametrize("pf", [0, 2, 3])
def test_extents_offsets_and_alignments(hip, pf):
    """Rectangle extents 1 .. 65 on both axes (at 4:4:4 the chroma planes have them too; at 4:2:0 / 4:2:2 theirs are the halves,
    rounded by the odd offsets), odd x and y with a reference at an odd address and pitch (byte loads on both sides), x = 16 with an
    aligned reference at a pitch of a multiple of 16 (16-byte loads on both sides where 16 columns fit), and x = 4 (dword loads)."""
    st = _state(hip, 96, 80, pf, 40 + pf)
    planes = st.ycbcr_out()
    for k, (w, h) in enumerate(EXTENTS):
        _check(st, (3, 5, w, h), BOTH, k, off=1, pad=3, planes=planes)
        _check(st, (16, 2, w, h), BOTH, 50 + k, off=0, pad=(-w) % 16 + (16 if k % 2 else 0), planes=planes)
        _check(st, (4, 7, w, h), BOTH, 90 + k, off=4, pad=(-w) % 4, planes=planes)
    st.close()


def test_whole_frame_each_metric_and_bufi(hip):
    st = _state(hip, 176, 144, 0, 3)
    planes = st.ycbcr_out()
    for flags in (cr.SSE, cr.SSIM, BOTH):
        _check(st, None, flags, flags, planes=planes)
        _check(st, None, flags, flags, bufi=0, planes=planes)
        _check(st, (0, 0, 176, 144), flags, flags, off=3, pad=1, planes=planes)
    ref = _device(_other(planes, 9))
    sse = _rec(st.compare(ref, "sse"))
    ssim = _rec(st.compare(ref, "ssim"))
    both = _rec(st.compare(ref, ("sse", "ssim")))
    assert sse[6:12] == [0] * 6 and ssim[0:6] == [0] * 6                 # the fields of the absent metric are 0
    assert sse[0:6] == both[0:6] and ssim[6:12] == both[6:12] and all(v > 0 for v in both)
    assert both[3:6] == [176 * 144, 88 * 72, 88 * 72] and both[9:12] == [43 * 35, 21 * 17, 21 * 17]
    st.close()


def test_several_work_groups_and_a_ragged_edge(hip):
    """600 x 402 at an odd corner of a 640 x 416 frame: 3 x 4 tiles of 240 x 120 with SSIM (the last of each row 120 wide, the last
    row 42 high), 3 x 4 of 256 x 128 without."""
    st = _state(hip, 640, 416, 0, 21)
    planes = st.ycbcr_out()
    for flags in (BOTH, cr.SSE):
        _check(st, (5, 7, 600, 402), flags, 4, off=0, pad=8, planes=planes)
        _check(st, (16, 8, 600, 402), flags, 5, off=0, pad=8, planes=planes)
    st.close()


def test_sums_are_64_bit(hip):
    """264 x 256 samples of 0 against 255: 4 394 649 600 > 2^32."""
    import torch
    st = _state(hip, 272, 256, 3, 0, fill=0)
    ref = [torch.full((256, 264), 255, dtype=torch.uint8, device="cuda") for _ in range(3)]
    res, blk = st.compare(ref, BOTH, (0, 0, 264, 256), blocks=True)
    rec = _rec(res)
    assert rec[0:3] == [4394649600] * 3 and rec[3:6] == [264 * 256] * 3
    assert rec[9:12] == [65 * 63] * 3 and rec[6:9] == [104 * 65 * 63] * 3         # (w = 104 for this window: the CPU test works it out)
    assert all(((b.cpu().numpy().astype(np.int64) & 0xFFFFFFFF) == 64 * 255 * 255).all() for b in blk)
    st.close()


@pytest.mark.parametrize("n", [8, 9])
def test_batches_are_chunked_and_reproducible(hip, n):
    import theora_amd
    import torch
    geom = [(176, 144, 0), (64, 48, 2), (48, 80, 3), (320, 240, 0), (16, 16, 0), (176, 144, 3), (128, 64, 2), (96, 96, 0), (272, 256, 0)][:n]
    states = [_state(hip, w, h, f, 100 + i) for i, (w, h, f) in enumerate(geom)]
    rects = [None if i % 2 else (3, 5, 11, 9) for i in range(n)]
    srcs = [cr.source_planes(s.ycbcr_out(), s.pixel_fmt, r) for s, r in zip(states, rects)]
    refs = [_other(src, i) for i, src in enumerate(srcs)]
    drefs = [_device(r, i % 3, i % 5) for i, r in enumerate(refs)]
    garbage = torch.iinfo(torch.int64).min + 12345
    results = [torch.full((12,), garbage, dtype=torch.int64, device="cuda") for _ in range(n)]      # overwritten, not added to
    theora_amd.picture_compare(states, drefs, results, ("sse", "ssim"), rects)
    again = [torch.full((12,), 77, dtype=torch.int64, device="cuda") for _ in range(n)]
    theora_amd.picture_compare(states, drefs, again, ("sse", "ssim"), rects)
    for i in range(n):
        assert _rec(results[i]) == cr.compare_planes(srcs[i], refs[i], BOTH), i
        assert _rec(again[i]) == _rec(results[i]), i                                                 # the same bytes twice
        assert _rec(states[i].compare(drefs[i], BOTH, rects[i])) == _rec(results[i]), i
    for s in states:
        s.close()


def _decode(hip, gst, geom, rng, ftype, keep):
    from theora_amd import synth
    fr = synth.gen_frame(geom, rng, ftype, "mixed", flimit=4)
    desc, ka = synth.upload_frame(synth.pack_frame(geom, fr))
    keep.append(ka)
    hip.decode_frames([gst], [desc])


def test_ordering_on_a_torch_stream(hip):
    """Decode, compare, decode on into the same state without a host wait: the result belongs to the frame compared."""
    import torch
    from theora_amd import synth
    w, h = 176, 144
    geom = synth.Geometry(w, h)
    rng = np.random.default_rng(11)
    gst = hip.State(w, h)
    keep = []
    _decode(hip, gst, geom, rng, hip.INTRA_FRAME, keep)
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)
    planes = gst.ycbcr_out()
    ref = _other(planes, 2)
    dref = _device(ref)
    s = torch.cuda.Stream()
    big = torch.zeros(32 << 20, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(8):           # keep the stream busy: the compare starts late
            big.add_(1)
        res = gst.compare(dref, BOTH, stream=s)
        after = res.clone()          # a torch op behind the call on the same stream
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)   # the second of these writes the buffer the compare reads
    _decode(hip, gst, geom, rng, hip.INTER_FRAME, keep)
    torch.cuda.synchronize()
    hip.synchronize()
    want = cr.compare_planes(planes, ref, BOTH)
    assert _rec(res) == want and _rec(after) == want
    assert _rec(gst.compare(dref, BOTH)) == cr.compare_planes(gst.ycbcr_out(), ref, BOTH) != want
    gst.close()


def test_refusals_leave_the_result_alone(hip):
    import torch
    from theora_amd import _lib
    L = _lib.load()
    a, fresh = _state(hip, 64, 48, 0, 1), hip.State(64, 48)
    ref = _device(_other(a.ycbcr_out(), 1))
    res = torch.full((13,), 7, dtype=torch.int64, device="cuda")
    blk = torch.zeros((6, 8), dtype=torch.int32, device="cuda")
    i64, vp = C.c_int64 * 3, C.c_void_p * 3

    def req(st, **kw):
        r = _lib.PictureCompareReq()
        r.state = st.handle if st is not None else None
        r.bufi, r.flags, r.result = -1, BOTH, res.data_ptr()
        for p in range(3):
            r.ref[p], r.ref_pitch[p] = ref[p].data_ptr(), ref[p].stride(0)
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    bad = [(_lib.EINVAL, req(a, flags=0)), (_lib.EINVAL, req(a, flags=4)), (_lib.EINVAL, req(a, flags=7)),
           (_lib.EINVAL, req(a, x=1, y=0, width=64, height=48)),                   # outside the frame
           (_lib.EINVAL, req(a, width=0, height=5)),
           (_lib.EINVAL, req(a, ref_pitch=i64(63, 32, 32))), (_lib.EINVAL, req(a, ref_pitch=i64(64, 32, 31))),
           (_lib.EINVAL, req(a, block_sse=vp(blk.data_ptr(), None, None), block_pitch=i64(7, 0, 0))),
           (_lib.EINVAL, req(a, result=res.data_ptr() + 4)),                       # misaligned
           (_lib.EINVAL, req(a, bufi=3)), (_lib.EINVAL, req(a, bufi=-2)),
           (_lib.EINVAL, req(fresh)),                                              # nothing decoded
           (_lib.EFAULT, req(a, result=None)),
           (_lib.EFAULT, req(a, ref=vp(ref[0].data_ptr(), None, ref[2].data_ptr()))),
           (_lib.EFAULT, req(None))]
    for want, r in bad:
        reqs = (_lib.PictureCompareReq * 2)(req(a), r)                             # all or nothing: the good one is not run either
        assert L.thip_picture_compare(reqs, 2, None) == want
        assert L.thip_picture_compare(C.byref(r), 1, None) == want
        hip.synchronize()
        assert (res == 7).all().item()
    assert L.thip_picture_compare(None, 1, None) == _lib.EFAULT and L.thip_picture_compare(C.byref(req(a)), -1, None) == _lib.EINVAL
    ok = req(a, block_sse=vp(blk.data_ptr(), None, None), block_pitch=i64(8, 0, 0))
    assert L.thip_picture_compare(C.byref(ok), 1, None) == 0
    hip.synchronize()
    assert _rec(res[:12]) == cr.compare_planes(a.ycbcr_out(), [r.cpu().numpy() for r in ref], BOTH) and res[12].item() == 7
    a.close()
    fresh.close()


# ---- th_decode_* ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,pf", [(176, 144, 0), (64, 48, 3)])
def test_decoder_picture_compare(hip, w, h, pf):
    from theora_amd.decoder import Decoder
    st = streamgen.Stream(w, h, pf, 31 + w + pf)
    dec = Decoder(st.header_packets())
    dec.set_host_output(False)
    for f in range(3):
        pkt, _ = st.frame(0 if f == 0 else 1, density=[0.9, 0.5, 0.15][f % 3])
        dec.packetin(pkt)
        for rect in (None, (3, 5, 37, 21)):
            planes = dec.ycbcr_out()
            src = cr.source_planes(planes, pf, rect)
            ref = _other(src, f)
            assert _rec(dec.picture_compare(_device(ref, f, f), ("sse", "ssim"), rect)) == cr.compare_planes(src, ref, BOTH), (f, rect)
        if f == 0:                      # a reference that is not the rectangle's size is refused before the device reads it
            with pytest.raises(ValueError):
                dec.picture_compare(_device([r[:-1] for r in ref]), "sse", rect)
            with pytest.raises(ValueError):
                dec.picture_compare(_device(ref), "sse", None)
        if f == 1:
            rc, _ = dec.packetin(b"")   # a dropped frame: TH_DUPFRAME, the same picture
            assert rc == 1
            assert _rec(dec.picture_compare(_device(ref), "sse", rect)) == cr.compare_planes(src, ref, cr.SSE)
    dec.close()


def test_decoder_picture_compare_before_the_first_frame(hip):
    from theora_amd import _lib
    from theora_amd.decoder import Decoder, PictureCompareArgs, TH_DECCTL_THIP_PICTURE_COMPARE
    st = streamgen.Stream(64, 48, 0, 3)
    dec = Decoder(st.header_packets())
    a = PictureCompareArgs()
    assert dec.ctl(TH_DECCTL_THIP_PICTURE_COMPARE, a, C.sizeof(a)) == _lib.EINVAL
    assert dec.ctl(TH_DECCTL_THIP_PICTURE_COMPARE, a, C.sizeof(a) - 4) == _lib.EINVAL
    assert dec.ctl(TH_DECCTL_THIP_PICTURE_COMPARE, None, 0) == _lib.EFAULT
    dec.close()


# ---- th_encode_* ----------------------------------------------------------------------------------------------------------
CONFIGS = {   # name: (Encoder arguments, {frame: duplicates})
    "key-only": (dict(quality=32), {}),
    "inter-5-modes": (dict(quality=32, inter=True, keyframe_interval=4), {}),
    "8-modes-block-qi": (dict(quality=28, inter=True, keyframe_interval=4, all_modes=True, block_qi=8), {}),
    "bitrate-drop": (dict(quality=32, inter=True, keyframe_interval=8, bitrate=2000, rate_flags=1), {}),     # TH_RATECTL_DROP_FRAMES
    "duplicate": (dict(quality=40, inter=True, keyframe_interval=4), {1: 2}),
}
GEOMETRIES = [(176, 144, None), (64, 48, (3, 5, 50, 38))]
NFRAMES = 4


def _rgb_frames(pw, ph, n, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (ph + 8, pw + 8, 3), dtype=np.uint8)
    base = (base // 4 + np.linspace(0, 180, pw + 8, dtype=np.int64)[None, :, None]).astype(np.uint8)
    return [np.ascontiguousarray(base[f:f + ph, 2 * f:2 * f + pw]) for f in range(n)]


def _sources(w, h, pic, kind):
    """Per frame: what goes into the encoder, and the picture-sized planes it is measured against."""
    from tests import enc_inter_ref, picture_in_ref
    x, y, pw, ph = pic or (0, 0, w, h)
    if kind == "rgb":
        rgb = _rgb_frames(pw, ph, NFRAMES, w)
        return rgb, [picture_in_ref.picture_in(im, 0, "rgb", x, y) for im in rgb]
    frames = enc_inter_ref.sequence("pan", w, h, 0, NFRAMES, seed=5)
    pics = [cr.source_planes(fr, 0, (x, y, pw, ph)) for fr in frames]
    return (frames if kind == "host" else pics), pics          # host: frame-sized planes; device: picture-sized ones


def _encode(w, h, pic, cfg, dups, inputs, kind, flags):
    """[(packet, granulepos, quality statistics or None)] of one run; flags 0: the switch stays off."""
    import torch
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT, TH_ENCCTL_THIP_SET_QUALITY_STATS, Encoder
    e = Encoder(w, h, 0, pic=pic, **cfg)
    if flags:
        e.set_quality_stats(flags)
    hdr = e.header_packets()
    out = []
    for f, x in enumerate(inputs):
        if dups.get(f):
            assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, dups[f])[0] == 0
        if kind == "rgb":
            t = torch.from_numpy(x).cuda()
            e.encode_rgb(t, "rgb")
            t.fill_(0)                        # the caller may overwrite its picture at once
        elif kind == "device":
            t = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in x]
            e.encode(t)
            for p in t:
                p.fill_(0)
        else:
            e.encode(x)
        while True:
            r = e.packetout(f == len(inputs) - 1)
            if r is None:
                break
            out.append((r[0], r[1], e.quality_stats() if flags else None))
    if flags:
        assert e.ctl(TH_ENCCTL_THIP_SET_QUALITY_STATS, 0)[0] == -10      # before the first frame only
    e.close()
    return hdr, out


@pytest.mark.parametrize("kind", ["host", "device", "rgb"])
@pytest.mark.parametrize("w,h,pic", GEOMETRIES, ids=["176x144", "50x38-odd"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_encoder_quality_statistics(hip, name, w, h, pic, kind):
    """The switch changes no packet, and sse / samples of every packet are numpy's over the packets decoded by this library's
    decoder (and by the reference decoder where it is built) against the source, over th_info's picture region; a dropped frame
    is measured against the picture held, a duplicate is not measured."""
    from oracle import ref as oref
    from theora_amd.decoder import Decoder
    cfg, dups = CONFIGS[name]
    inputs, pics = _sources(w, h, pic, kind)
    rect = pic or (0, 0, w, h)
    flags = BOTH if name != "inter-5-modes" else cr.SSE
    hdr_off, off = _encode(w, h, pic, cfg, dups, inputs, kind, 0)
    hdr, on = _encode(w, h, pic, cfg, dups, inputs, kind, flags)
    assert hdr == hdr_off and [(p, g) for p, g, _ in on] == [(p, g) for p, g, _ in off]
    decs = [Decoder(hdr)] + ([oref.RefDecoder(hdr)] if oref.available() else [])
    frame, measured, empties = -1, [], 0
    left = 0
    for pkt, _, q in on:
        dup = left > 0
        if dup:
            left -= 1
        else:
            frame += 1
            left = dups.get(frame, 0)
        assert q["flags"] == flags and q["measured"] == int(not dup)
        empties += len(pkt) == 0 and not dup
        for d in decs:
            d.packetin(pkt)
            if dup:
                assert q["sse"] == q["samples"] == q["ssim_q20"] == q["windows"] == [0, 0, 0]
                continue
            want = cr.compare(d.ycbcr_out(), 0, pics[frame], flags, rect)
            assert q["sse"] + q["samples"] + q["ssim_q20"] + q["windows"] == want, (frame, type(d).__name__)
            assert q["psnr"][0] == pytest.approx(cr.psnr(want[0], want[3])) and q["compare_ms"] > 0
        measured.append(q["measured"])
    assert frame == NFRAMES - 1 and sum(measured) == NFRAMES and len(on) == NFRAMES + sum(dups.values())
    if name == "bitrate-drop":
        assert empties >= 1          # the controller dropped a frame, and it was measured
    for d in decs:
        d.close()
