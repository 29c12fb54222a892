"""th_encode_* with activity masking on the GPU (TH_ENCCTL_THIP_SET_MASKING): the packets and the mask statistics equal
tests/enc_mask_ref.py's restatement byte for byte -- key-only streams and inter frames with five and eight modes, the three pixel
formats, an odd picture region, qualities 0 / 32 / 63 with two and three qi -- and so they do crossed with bitrate mode, the device
packetiser, R'G'B' input, automatic key frames and the quality statistics; masking without block qi is the plain stream, masking 0
is block qi alone."""
import numpy as np
import pytest

from tests import enc_bqi_ref as B
from tests import enc_cut_ref as CR
from tests import enc_mask_ref as K
from tests import enc_modes_ref as M
from tests import enc_rate_ref as RR
from tests import enc_ref
from tests.test_gpu_encoder_bqi import _frames

pytestmark = pytest.mark.gpu

MASK_FIELDS = ("ratio", "measured", "activity_avg", "activity_max")


def _encode(w, h, fmt, quality, frames, delta, k, pic=None, inter=False, modes=False, kf=64, dev=False, rgb=False, **kw):
    """Headers, and per packet a dict: pkt, gp, mask, bqi, rate (bitrate mode), cut, quality (with quality statistics)."""
    from theora_amd.encoder import Encoder
    quality_stats = kw.pop("quality_stats", False)
    if inter:
        kw.update(inter=True, keyframe_interval=kf, all_modes=modes)
    e = Encoder(w, h, fmt, quality, pic=pic, block_qi=delta, masking=k, **kw)
    if quality_stats:
        e.set_quality_stats(("sse", "ssim"))
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if rgb:
            e.encode_rgb(fr, "rgb")
        elif dev:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], gp=r[1], mask=e.mask_stats(), bqi=e.block_qi_stats(), cut=e.cut_stats(),
                            rate=e.rate_stats() if kw.get("bitrate") else None, quality=e.quality_stats() if quality_stats else None,
                            pack=e.pack_stats()))
    e.close()
    return hdr, out


def _same_mask(got, want):
    assert {n: got[n] for n in MASK_FIELDS} == want, (got, want)
    assert got["mask_ms"] > 0 if want["measured"] else got["mask_ms"] == 0


CASES = [   # (w, h, fmt, pic, quality, delta, k, content, inter, eight modes, device input)
    (64, 48, 0, None, 32, 8, 4, "pan", False, False, False),          # nqis 3
    (64, 48, 2, None, 0, 6, 2, "shear", False, False, True),          # nqis 2 at the bottom
    (64, 48, 3, None, 63, 10, 16, "uncover", False, False, False),    # nqis 2 at the top
    (80, 64, 0, (5, 3, 67, 49), 32, 12, 4, "pan", False, False, False),
    (80, 64, 2, (5, 3, 67, 49), 63, 7, 16, "pan", True, False, True),
    (80, 64, 3, (5, 3, 67, 49), 0, 9, 2, "shear", True, True, False),
    (64, 48, 0, None, 32, 8, 4, "pan", True, False, False),
    (64, 48, 2, None, 63, 31, 2, "shear", True, True, True),
    (176, 144, 0, None, 32, 8, 4, "pan", False, False, False),
    (176, 144, 0, None, 0, 8, 16, "pan", True, False, True),
    (176, 144, 3, None, 32, 8, 4, "shear", True, True, False),
    (176, 144, 2, None, 63, 8, 2, "uncover", True, True, False),
]


@pytest.mark.parametrize("w,h,fmt,pic,quality,delta,k,kind,inter,modes,dev", CASES)
def test_mask_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, delta, k, kind, inter, modes, dev):
    frames = _frames(kind, w, h, fmt, 3, pic)
    kf = 64 if inter else 1
    hdr, out = _encode(w, h, fmt, quality, frames, delta, k, pic=pic, inter=inter, modes=modes, kf=kf, dev=dev)
    ref = K.MaskEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6, delta, k, modes=modes)
    changed = 0
    try:
        assert len(out) == len(frames)
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            g = out[f]
            _same_mask(g["mask"], want["mask"])
            assert g["bqi"] == want["bqi"], (f, g["bqi"], want["bqi"])
            assert g["pkt"] == want["packet"], (f, len(g["pkt"]), len(want["packet"]))
            changed += want["mask"]["measured"]
    finally:
        ref.close()
    assert changed >= 1


def _rgb_frames(w, h, n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 2 + yy, 255 - xx - yy // 2, (xx * yy) // 16], 2) % 256
    base[:, w // 2:] = rng.integers(0, 256, (h, w - w // 2, 3))
    return [np.ascontiguousarray(np.roll(base, 2 * f, 1)).astype(np.uint8) for f in range(n)]


@pytest.mark.parametrize("cross", ["device_pack", "rgb", "auto_keyframes", "quality_stats"])
def test_crossings_equal_the_restatement(hip, cross):
    from tests import picture_in_ref
    w, h, fmt, q, delta, k = 176, 144, 0, 32, 8, 4
    setup_of = lambda hdr: enc_ref.SetupParams(hdr[2])   # noqa: E731
    if cross == "rgb":
        pic = (5, 3, 167, 139)
        images = _rgb_frames(pic[2], pic[3], 3, 2)
        frames = [picture_in_ref.picture_in(im, fmt, "rgb", pic[0], pic[1]) for im in images]
        hdr, out = _encode(w, h, fmt, q, images, delta, k, pic=pic, inter=True, kf=64, rgb=True)
        ref = K.MaskEncoder(w, h, fmt, pic, setup_of(hdr), 64, 6, delta, k)
    elif cross == "auto_keyframes":
        class CutMaskEncoder(K.MaskEncoder, CR.CutBase):
            pass
        frames = CR.scene(w, h, fmt, 4, 2)
        hdr, out = _encode(w, h, fmt, q, frames, delta, k, inter=True, kf=64, auto_keyframes=CR.RECOMMENDED)
        ref = CutMaskEncoder(w, h, fmt, (0, 0, w, h), setup_of(hdr), 64, 6, delta, k)
        ref.t = CR.RECOMMENDED
    else:
        frames = M.sequence("shear", w, h, fmt, 3, seed=6)
        sw = dict(device_pack=True) if cross == "device_pack" else dict(quality_stats=True)
        hdr, out = _encode(w, h, fmt, q, frames, delta, k, inter=True, modes=True, kf=64, **sw)
        ref = K.MaskEncoder(w, h, fmt, (0, 0, w, h), setup_of(hdr), 64, 6, delta, k, modes=True)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, q)
            _same_mask(out[f]["mask"], want["mask"])
            assert out[f]["pkt"] == want["packet"], (f, len(out[f]["pkt"]), len(want["packet"]))
            if cross == "auto_keyframes":
                assert out[f]["cut"]["cut"] == want["cut"]["cut"] == int(f == 2)
            if cross == "device_pack":
                assert out[f]["pack"]["device"] == 1
            if cross == "quality_stats":
                assert out[f]["quality"]["measured"] == 1 and out[f]["quality"]["sse"][0] > 0
    finally:
        ref.close()


@pytest.mark.parametrize("modes", [False, True], ids=["five_modes", "eight_modes"])
def test_bitrate_mode_equals_the_restatement(hip, modes):
    """The probe and the controller are unchanged: the qi sequence, the controller's record and the packets are those of the rate
    restatement around the masked encoder."""
    w, h, fmt, bitrate, delta, k = 176, 144, 0, 300000, 8, 4
    frames = M.sequence("shear" if modes else "pan", w, h, fmt, 4, seed=8)
    hdr, out = _encode(w, h, fmt, 32, frames, delta, k, inter=True, modes=modes, kf=64, bitrate=bitrate)
    rs = RR.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, inter=True, kf_interval=64)
    rs.enc.close()
    rs.enc = K.MaskEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6, delta, k, modes=modes)
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
        assert g["mask"]["measured"] == int(bool(wpkt)) and g["mask"]["ratio"] == k


def test_masking_without_block_qi_and_masking_zero(hip):
    """Masking on with block qi off: the plain stream's packets, measured = 0.  Masking 0: block qi alone.  And the quality
    statistics change no packet of a masked stream."""
    w, h, fmt, q = 64, 48, 0, 30
    frames = M.sequence("shear", w, h, fmt, 3, seed=3)
    kw = dict(inter=True, modes=True, kf=64)
    plain = _encode(w, h, fmt, q, frames, 0, 0, **kw)
    nobqi = _encode(w, h, fmt, q, frames, 0, 4, **kw)
    assert plain[0] == nobqi[0] and [g["pkt"] for g in plain[1]] == [g["pkt"] for g in nobqi[1]]
    for g in nobqi[1]:
        assert g["mask"] == dict(ratio=4, measured=0, activity_avg=0, activity_max=0, mask_ms=0.0)
    bqi = _encode(w, h, fmt, q, frames, 8, 0, **kw)
    ref = B.BqiEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(bqi[0][2]), 64, 6, 8, modes=True)
    try:
        for fr, g in zip(frames, bqi[1]):
            assert g["pkt"] == ref.frame(fr, q)["packet"]
            assert g["mask"] == dict(ratio=0, measured=0, activity_avg=0, activity_max=0, mask_ms=0.0)
    finally:
        ref.close()
    masked = _encode(w, h, fmt, q, frames, 8, 4, **kw)
    watched = _encode(w, h, fmt, q, frames, 8, 4, quality_stats=True, **kw)
    assert [g["pkt"] for g in masked[1]] == [g["pkt"] for g in watched[1]]
    assert [g["pkt"] for g in masked[1]] != [g["pkt"] for g in bqi[1]]       # and masking does change them


def test_masking_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_MASKING, Encoder
    e = Encoder(64, 48, 0, 30, block_qi=4, masking=4)
    e.header_packets()
    e.encode(M.sequence("pan", 64, 48, 0, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_MASKING, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_MASKING, 4)[0] == -10
    assert e.mask_stats()["measured"] == 1
    e.close()
