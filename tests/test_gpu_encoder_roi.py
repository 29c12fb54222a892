"""th_encode_* with a region-of-interest map on the GPU (TH_ENCCTL_THIP_SET_ROI_MAP): the packets and the ROI statistics equal
tests/enc_roi_ref.py's restatement byte for byte -- key-only streams and inter streams with five and eight modes at 64 x 48, 80 x 64
with an odd picture region and 176 x 144, crossed with masking, the skip decision and the level choice, with bitrate mode, the device
packetiser, R'G'B' input and a map that is a device tensor --; a map changed and cleared between frames; the zero map and block qi
off give the plain stream; the map moves the picture's error the way it says; and the reference decoder plays the stream."""
import numpy as np
import pytest

from tests import enc_modes_ref as M
from tests import enc_ref
from tests import enc_rdq_ref as Q
from tests import enc_roi_ref as R
from tests import refcmp
from tests.test_gpu_encoder_bqi import _frames

pytestmark = pytest.mark.gpu

FIELDS = ("active", "measured", "map_width", "map_height", "exp_min", "exp_max", "exp_sum", "scale_min", "scale_max", "clamped")


def _encode(w, h, fmt, quality, frames, rois, delta=8, k=0, pic=None, kf=1, modes=False, skip=False, rdq=0, rgb=False, tensor=False,
            decode=False, **kw):
    """Headers, and per packet a dict: pkt, roi, mask, pack, rate (bitrate mode), picture (decode: the Decoder's luma).  rois: the
    map in force for each frame (None: cleared); it is set again only where it changes."""
    from theora_amd.encoder import Encoder
    inter = kf != 1
    e = Encoder(w, h, fmt, quality, pic=pic, inter=inter, keyframe_interval=kf if inter else None, all_modes=modes and inter,
                block_qi=delta, masking=k, rd_skip=skip and inter, rd_quant=rdq, **kw)
    hdr = e.header_packets()
    dec = None
    if decode:
        from theora_amd.decoder import Decoder
        dec = Decoder(hdr)
    out, last = [], None
    for f, fr in enumerate(frames):
        roi = rois[f]
        if f == 0 or roi is not last:
            if tensor and roi is not None:
                import torch
                side = torch.cuda.Stream()
                with torch.cuda.stream(side):
                    t = torch.from_numpy(np.ascontiguousarray(roi)).cuda()
                    e.set_roi(t, stream=side)
                    t.fill_(99)   # the caller's tensor is its own again as soon as the call returns, on its stream
            elif f or roi is not None:
                e.set_roi(roi)
            last = roi
        if rgb:
            e.encode_rgb(fr, "rgb")
        else:
            e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            g = dict(pkt=r[0], roi=e.roi_stats(), mask=e.mask_stats(), pack=e.pack_stats(), rate=e.rate_stats() if kw.get("bitrate") else None)
            if dec is not None:
                dec.packetin(r[0])
                g["picture"] = np.array(dec.ycbcr_out()[0])
            out.append(g)
    e.close()
    if dec is not None:
        dec.close()
    return hdr, out


def _same_roi(got, want):
    assert {n: got[n] for n in FIELDS} == want, (got, want)
    assert got["roi_ms"] > 0 if want["measured"] else got["roi_ms"] == 0


def _maps(rng, pic, n):
    """n maps for a picture: the macro-block grid, a coarse one, one at pixel resolution with a pitch of its own."""
    pw, ph = pic[2], pic[3]
    big = rng.integers(-64, 65, (ph, pw + 3)).astype(np.int8)
    pool = [rng.integers(-64, 65, ((ph + 15) // 16, (pw + 15) // 16)).astype(np.int8), rng.integers(-64, 65, (2, 3)).astype(np.int8),
            big[:, :pw]]
    return [pool[f % 3] for f in range(n)]


CASES = [   # (w, h, fmt, pic, quality, delta, masking, content, key-frame interval, eight modes, skip, rd_quant)
    (64, 48, 0, None, 32, 8, 0, "pan", 1, False, False, 0),
    (64, 48, 2, None, 32, 8, 4, "pan", 1, False, False, 5),
    (80, 64, 3, (5, 3, 67, 49), 40, 12, 0, "shear", 1, False, False, 0),
    (64, 48, 0, None, 32, 8, 0, "pan", 64, False, False, 0),
    (64, 48, 3, None, 24, 8, 4, "shear", 64, True, True, 3),
    (80, 64, 0, (5, 3, 67, 49), 32, 12, 4, "pan", 64, False, True, 0),
    (80, 64, 2, (5, 3, 67, 49), 32, 10, 0, "shear", 64, True, False, 5),
    (176, 144, 0, None, 32, 8, 0, "pan", 1, False, False, 3),
    (176, 144, 0, None, 32, 8, 4, "shear", 64, True, True, 3),
    (176, 144, 2, None, 40, 8, 0, "pan", 64, False, True, 0),
]


def _ref(w, h, fmt, pic, hdr, kf, delta, k, modes, skip, rdq):
    inter = kf != 1
    return R.RoiEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6, delta, k, modes and inter, False,
                        skip and inter, rdq)


def _compare(out, ref, frames, rois, q):
    assert len(out) == len(frames)
    used = 0
    for f, fr in enumerate(frames):
        want = ref.frame(fr, q, roi=rois[f])
        _same_roi(out[f]["roi"], want["roi"])
        assert {n: out[f]["mask"][n] for n in want["mask"]} == want["mask"], f
        assert out[f]["pkt"] == want["packet"], (f, len(out[f]["pkt"]), len(want["packet"]))
        used += want["roi"]["measured"]
    return used


@pytest.mark.parametrize("w,h,fmt,pic,q,delta,k,kind,kf,modes,skip,rdq", CASES)
def test_roi_packets_equal_the_restatement(hip, w, h, fmt, pic, q, delta, k, kind, kf, modes, skip, rdq):
    frames = _frames(kind, w, h, fmt, 3, pic)
    rois = _maps(np.random.default_rng(w + fmt + kf), pic or (0, 0, w, h), 3)
    hdr, out = _encode(w, h, fmt, q, frames, rois, delta, k, pic=pic, kf=kf, modes=modes, skip=skip, rdq=rdq)
    ref = _ref(w, h, fmt, pic, hdr, kf, delta, k, modes, skip, rdq)
    try:
        assert _compare(out, ref, frames, rois, q) == 3
    finally:
        ref.close()


@pytest.mark.parametrize("cross", ["device_pack", "rgb", "tensor"])
def test_crossings_equal_the_restatement(hip, cross):
    from tests import picture_in_ref
    from tests.test_gpu_encoder_mask import _rgb_frames
    w, h, fmt, q, delta, k = 176, 144, 0, 32, 8, 4
    pic = (5, 3, 167, 139) if cross == "rgb" else None
    rois = _maps(np.random.default_rng(11), pic or (0, 0, w, h), 3)
    if cross == "rgb":
        images = _rgb_frames(pic[2], pic[3], 3, 2)
        frames = [picture_in_ref.picture_in(im, fmt, "rgb", pic[0], pic[1]) for im in images]
        hdr, out = _encode(w, h, fmt, q, images, rois, delta, k, pic=pic, kf=64, rgb=True)
    else:
        frames = M.sequence("shear", w, h, fmt, 3, seed=6)
        hdr, out = _encode(w, h, fmt, q, frames, rois, delta, k, kf=64, modes=True, skip=True, rdq=3, device_pack=cross == "device_pack",
                           tensor=cross == "tensor")
    ref = _ref(w, h, fmt, pic, hdr, 64, delta, k, cross != "rgb", cross != "rgb", 0 if cross == "rgb" else 3)
    try:
        assert _compare(out, ref, frames, rois, q) == 3
    finally:
        ref.close()
    if cross == "device_pack":
        assert all(g["pack"]["device"] == 1 for g in out)


def test_bitrate_mode_equals_the_restatement(hip):
    """The probe and the controller are unchanged: the qi sequence, the controller's record and the packets are those of the rate
    restatement around the map's encoder."""
    w, h, fmt, bitrate, delta = 96, 64, 0, 60000, 8
    frames = Q.S.clip("static", w, h, fmt, 4, seed=8)
    roi = np.random.default_rng(4).integers(-64, 65, (4, 6)).astype(np.int8)
    hdr, out = _encode(w, h, fmt, 32, frames, [roi] * 4, delta, 0, kf=64, modes=True, skip=True, rdq=5, bitrate=bitrate)
    rs = Q.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, kf_interval=64, delta=delta, w=5)
    rs.enc.close()
    rs.enc = _ref(w, h, fmt, None, hdr, 64, delta, 0, True, True, 5)
    rs.enc.roi = roi
    want = []
    try:
        for fr in frames:
            want.extend(rs.frame(fr))
    finally:
        rs.close()
    assert len(out) == len(want)
    for n, (g, (wpkt, rec)) in enumerate(zip(out, want)):
        for name, v in rec.items():
            assert g["rate"][name] == v, (n, name, g["rate"][name], v)
        assert g["pkt"] == wpkt, n
        assert g["roi"]["measured"] == int(bool(wpkt)) and g["roi"]["active"] == 1


def test_a_map_changed_and_cleared_between_frames(hip):
    w, h, fmt, q = 64, 48, 0, 32
    frames = M.sequence("pan", w, h, fmt, 5, seed=2)
    rng = np.random.default_rng(5)
    a, b = rng.integers(-64, 65, (3, 4)).astype(np.int8), rng.integers(-64, 65, (48, 64)).astype(np.int8)
    rois = [None, a, b, None, a]
    hdr, out = _encode(w, h, fmt, q, frames, rois, 8, 4, kf=64, modes=True)
    ref = _ref(w, h, fmt, None, hdr, 64, 8, 4, True, False, 0)
    try:
        assert _compare(out, ref, frames, rois, q) == 3
    finally:
        ref.close()
    assert [g["roi"]["active"] for g in out] == [0, 1, 1, 0, 1] and [g["roi"]["map_width"] for g in out] == [0, 4, 64, 0, 4]


def test_the_zero_map_and_block_qi_off_give_the_plain_stream(hip):
    w, h, fmt, q = 64, 48, 0, 30
    frames = M.sequence("shear", w, h, fmt, 3, seed=3)
    busy = np.random.default_rng(6).integers(-64, 65, (3, 4)).astype(np.int8)
    kw = dict(kf=64, modes=True, skip=True, rdq=3)
    for delta, k in ((8, 0), (8, 4), (0, 0)):
        plain = _encode(w, h, fmt, q, frames, [None] * 3, delta, k, **kw)
        zero = _encode(w, h, fmt, q, frames, [np.zeros((3, 4), np.int8)] * 3, delta, k, **kw)
        assert plain[0] == zero[0] and [g["pkt"] for g in plain[1]] == [g["pkt"] for g in zero[1]], (delta, k)
        assert all(g["roi"]["measured"] == int(bool(delta)) and g["roi"]["active"] == 1 for g in zero[1])
        assert all(g["roi"]["measured"] == 0 and g["roi"]["active"] == 0 and g["roi"]["roi_ms"] == 0 for g in plain[1])
        if delta:
            assert all((g["roi"]["exp_min"], g["roi"]["exp_max"], g["roi"]["exp_sum"]) == (0, 0, 0) for g in zero[1])
        mapped = _encode(w, h, fmt, q, frames, [busy] * 3, delta, k, **kw)
        assert ([g["pkt"] for g in mapped[1]] != [g["pkt"] for g in plain[1]]) == bool(delta)   # and a map does change them


def test_float_maps_and_out_of_range_entries(hip):
    """A float map is octaves: clamp(round(16 x), -64, 64), on the host and on the device.  An int8 tensor's entries outside -64..64
    are clamped on the device and counted; a host map's are refused, and the map in force stays."""
    import torch
    w, h, fmt, q = 64, 48, 0, 32
    frames = M.sequence("pan", w, h, fmt, 1, seed=2)
    x = np.random.default_rng(8).uniform(-5, 5, (6, 8))
    v = R.from_octaves(x)
    assert v.min() == -64 and v.max() == 64
    want = _encode(w, h, fmt, q, frames, [v])[1][0]
    for m in (x, x.astype(np.float32), torch.from_numpy(x).cuda(), torch.from_numpy(x.astype(np.float32)).cuda().half()):
        got = _encode(w, h, fmt, q, frames, [m])[1][0]
        if isinstance(m, torch.Tensor) and m.dtype == torch.float16:
            continue   # (half rounds 16 x differently near a tie: only that it is taken)
        assert got["pkt"] == want["pkt"] and {n: got["roi"][n] for n in FIELDS} == {n: want["roi"][n] for n in FIELDS}
    wild = v.astype(np.int16) * 2
    wild[0, 0] = 0
    nbad = int((np.abs(wild) > 64).sum())
    assert nbad > 10
    t = torch.from_numpy(np.clip(wild, -128, 127).astype(np.int8)).cuda()
    got = _encode(w, h, fmt, q, frames, [t])[1][0]
    clamped = _encode(w, h, fmt, q, frames, [np.clip(wild, -64, 64).astype(np.int8)])[1][0]
    assert got["pkt"] == clamped["pkt"] and got["roi"]["clamped"] == nbad and clamped["roi"]["clamped"] == 0
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, q, block_qi=8)
    e.header_packets()
    e.set_roi(v)
    with pytest.raises(ValueError):
        e.set_roi(np.clip(wild, -128, 127).astype(np.int8))
    e.encode(frames[0])
    with pytest.raises(ValueError):
        e.set_roi(v)           # not with a frame pending
    assert e.packetout(True)[0] == want["pkt"] and e.roi_stats()["map_width"] == 8
    e.close()


def _halves(picture, source):
    d = (picture.astype(np.int64) - source.astype(np.int64)) ** 2
    half = source.shape[1] // 2
    return int(d[:, :half].sum()), int(d[:, half:].sum())


def test_the_picture_moves_the_way_the_map_says(hip):
    """The 176 x 144 "pan" key frame (tests/enc_inter_ref.sequence, seed 21) at quality 32, delta 12, the left half at v = +32 and the
    right half at -32, decoded through Decoder and compared with the same encoder without a map: the left half's luma SSE falls and
    the right half's rises.  The restatement shows both on the CPU first (tests/test_encoder_roi_cpu.py's test of the same name):
    without the map 1198 bytes, SSE 143878 left and 86479 right; with it 1947 bytes, 102896 left and 92605 right."""
    from tests import enc_inter_ref as IR
    w, h = 176, 144
    planes = IR.sequence("pan", w, h, 0, 1, seed=21)
    roi = np.array([[32, -32]], np.int8)
    off = _encode(w, h, 0, 32, planes, [None], 12, decode=True)[1][0]
    on = _encode(w, h, 0, 32, planes, [roi], 12, decode=True)[1][0]
    a, b = _halves(off["picture"], planes[0][0]), _halves(on["picture"], planes[0][0])
    print("\nwithout the map: %d bytes, SSE left %d right %d; with it: %d bytes, left %d right %d" % ((len(off["pkt"]),) + a + (len(on["pkt"]),) + b))
    assert b[0] < a[0] and b[1] > a[1]


def test_the_reference_decoder_plays_a_stream_with_a_map(hip):
    """The packets of a stream coded with maps go through the reference decoder: none refused, and its pictures are the encoder's own
    reconstruction."""
    from oracle import ref
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    w, h, fmt, q = 80, 64, 0, 32
    pic = (5, 3, 67, 49)
    frames = _frames("shear", w, h, fmt, 4, pic)
    rois = _maps(np.random.default_rng(12), pic, 4)
    e = Encoder(w, h, fmt, q, pic=pic, inter=True, keyframe_interval=64, all_modes=True, block_qi=10, masking=4, rd_skip=True, rd_quant=3)
    hdr = e.header_packets()
    dec = ref.RefDecoder(hdr)
    try:
        for f, fr in enumerate(frames):
            e.set_roi(rois[f])
            e.encode(fr)
            r = e.packetout(f == len(frames) - 1)
            assert e.roi_stats()["measured"] == 1
            assert dec.packetin(r[0])[0] == 0, f
            got, want = dec.ycbcr_out(), e.recon()
            for p in range(3):
                assert np.array_equal(np.asarray(got[p]), want[p]), (f, p)
    finally:
        dec.close()
        e.close()
