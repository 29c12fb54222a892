"""th_encode_* with block-level qi on the GPU (TH_ENCCTL_THIP_SET_BLOCK_QI): the packets and statistics equal tests/enc_bqi_ref.py's
restatement byte for byte (key frames in every pixel format and an odd picture region, inter frames with five and eight modes, host
and device input), delta 0 is the plain encoder, th_decode_* reproduces the reconstruction, bitrate mode holds its bounds, FFmpeg plays
a clip with three qi, and the choice lowers the real rate-distortion cost and the bytes at matched PSNR."""
import numpy as np
import pytest

from tests import enc_bqi_ref as B
from tests import enc_inter_ref as IR
from tests import enc_modes_ref as M
from tests import enc_ref
from tests.test_thirdparty_decoder import browser  # noqa: F401 -- the fixture (skips where that browser cannot run)


def _frames(kind, w, h, fmt, n, pic, seed=0):
    frames = M.sequence(kind, w, h, fmt, n, seed=seed)
    if pic is None:
        return frames
    return [[a[y0:y0 + ch, x0:x0 + cw] for a, (x0, y0, cw, ch) in zip(fr, [enc_ref.chroma_region(pic, fmt, p) for p in range(3)])]
            for fr in frames]


def _encode(w, h, fmt, quality, frames, delta, pic=None, inter=False, modes=False, kf=64, device_input=False):
    """Headers, and per packet (bytes, granulepos, block-qi stats, frame stats, recon or None)."""
    from theora_amd.encoder import Encoder
    kw = dict(inter=True, keyframe_interval=kf, all_modes=modes) if inter else {}
    e = Encoder(w, h, fmt, quality, pic=pic, block_qi=delta, **kw)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if device_input:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        r = e.packetout(f == len(frames) - 1)
        out.append((r[0], r[1], e.block_qi_stats(), e.stats(), e.recon() if inter else None))
    e.close()
    return hdr, out


CASES = [   # (w, h, fmt, pic, quality, delta, content, inter, eight modes, device input, frames)
    (64, 48, 0, None, 32, 8, "pan", False, False, False, 3),
    (64, 48, 2, None, 40, 6, "shear", False, False, True, 2),
    (64, 48, 3, None, 20, 10, "uncover", False, False, False, 2),
    (64, 48, 0, (1, 2, 61, 45), 63, 12, "pan", False, False, False, 2),
    (64, 48, 2, (1, 2, 61, 45), 0, 7, "pan", False, False, True, 2),
    (96, 64, 0, None, 32, 8, "pan", True, False, False, 5),
    (96, 64, 2, (1, 2, 93, 61), 24, 5, "cut", True, False, True, 5),
    (96, 64, 0, None, 40, 8, "shear", True, True, False, 5),
    (96, 64, 3, None, 28, 31, "uncover", True, True, True, 5),
    # the smallest frames at which the geometry can go wrong, in every pixel format, a key frame and two inter frames with all
    # eight modes: one macro block (every super block partial; a 1x1 chroma plane at 4:2:0), and 6x10 luma fragments over 3x5
    # chroma fragments at 4:2:0 (super blocks partial in both directions, odd chroma counts)
    (16, 16, 0, None, 48, 3, "pan", True, True, False, 3),
    (16, 16, 2, None, 40, 5, "shear", True, True, False, 3),
    (16, 16, 3, None, 32, 6, "uncover", True, True, True, 3),
    (48, 80, 0, None, 36, 8, "uncover", True, True, False, 3),
    (48, 80, 2, None, 28, 6, "shear", True, True, True, 3),
    (48, 80, 3, None, 44, 10, "pan", True, True, False, 3),
]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,delta,kind,inter,modes,dev,n", CASES)
def test_bqi_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, delta, kind, inter, modes, dev, n):
    frames = _frames(kind, w, h, fmt, n, pic)
    kf = 4 if inter else 1
    hdr, out = _encode(w, h, fmt, quality, frames, delta, pic=pic, inter=inter, modes=modes, kf=kf, device_input=dev)
    ref = B.BqiEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6, delta, modes=modes)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            pkt, gp, bs, st, rec = out[f]
            assert bs == want["bqi"], (f, bs, want["bqi"])
            assert pkt == want["packet"], (f, len(pkt), len(want["packet"]))
            if rec is not None:
                for p in range(3):
                    assert np.array_equal(rec[p], ref.recon[p]), (f, p)
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inter,modes", [(False, False), (True, False), (True, True)])
def test_delta_zero_is_the_plain_encoder(hip, inter, modes):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_BLOCK_QI, Encoder
    w, h = 96, 64
    frames = M.sequence("shear", w, h, 0, 4, seed=3)
    outs = []
    for call in (False, True):
        kw = dict(inter=True, keyframe_interval=4, all_modes=modes) if inter else {}
        e = Encoder(w, h, 0, 30, **kw)
        if call:
            assert e.ctl(TH_ENCCTL_THIP_SET_BLOCK_QI, 9)[0] == 0
            assert e.ctl(TH_ENCCTL_THIP_SET_BLOCK_QI, 0)[0] == 0
        hdr = e.header_packets()
        pk = []
        for f, fr in enumerate(frames):
            e.encode(fr)
            pk.append(e.packetout(f == 3)[:2])
            bs = e.block_qi_stats()
            if pk[-1][0]:
                assert bs["nqis"] == 1 and bs["qis"] == [30, 0, 0] and bs["flag_bits"] == 0
                assert sum(bs["blocks"][1]) == sum(bs["blocks"][2]) == 0
        e.close()
        outs.append((hdr, pk))
    assert outs[0] == outs[1]


@pytest.mark.gpu
def test_block_qi_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_BLOCK_QI, Encoder
    e = Encoder(64, 48, 0, 30, inter=True, block_qi=4)
    e.header_packets()
    e.encode(M.sequence("pan", 64, 48, 0, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_BLOCK_QI, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_BLOCK_QI, 4)[0] == -10
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("modes,fmt", [(False, 0), (True, 2)])
def test_recon_is_the_decoders_picture(hip, modes, fmt):
    """th_decode_* of the packets gives the encoder's reconstruction, and the oracle (through the restatement above) agrees."""
    from theora_amd.decoder import Decoder
    w, h, q = 176, 144, 32
    frames = M.sequence("shear" if modes else "pan", w, h, fmt, 6, seed=5)
    hdr, out = _encode(w, h, fmt, q, frames, 10, inter=True, modes=modes, kf=4)
    assert all(o[2]["nqis"] == 3 for o in out if o[0])
    assert any(sum(o[2]["blocks"][1]) + sum(o[2]["blocks"][2]) for o in out)   # some blocks leave qis[0]
    dec = Decoder(hdr)
    try:
        for f, (pkt, gp, bs, st, rec) in enumerate(out):
            rc, dgp = dec.packetin(pkt)
            assert dgp == gp
            pic = dec.ycbcr_out()
            for p in range(3):
                assert np.array_equal(rec[p], pic[p]), (f, p)
    finally:
        dec.close()


@pytest.mark.gpu
def test_bitrate_mode_holds_its_target_with_block_qi(hip):
    """test_gpu_encoder_rate.test_rate_holds_its_target's bounds on a shorter pan (60 frames, middle target) with block qi 8."""
    from theora_amd.encoder import Encoder
    w, h, n = 352, 288, 60
    frames = IR.sequence("pan", w, h, 0, n, seed=21)

    def clip_bytes(q):
        e = Encoder(w, h, 0, q, inter=True, keyframe_interval=64)
        e.header_packets()
        tot = 0
        for f, fr in enumerate(frames):
            e.encode(fr)
            tot += len(e.packetout(f == n - 1)[0])
        e.close()
        return tot
    lo, hi = clip_bytes(8) * 8 * 30 // n, clip_bytes(56) * 8 * 30 // n
    e = Encoder(w, h, 0, 32, inter=True, keyframe_interval=12, bitrate=(lo + hi) // 2, rate_buffer=12, block_qi=8)
    e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        while True:
            r = e.packetout(f == n - 1)
            if r is None:
                break
            out.append((r[0], e.rate_stats(), e.block_qi_stats()))
    e.close()
    T = out[0][1]["target"]
    Rr = 12 * T
    total, last_qi = 0, None
    for pkt, st, bs in out:
        total += 8 * len(pkt)
        if not st["dropped"] and not st["duplicate"]:
            last_qi = st["qi"]
            if pkt:
                assert bs["qis"][0] == st["qi"] and bs["nqis"] >= 2
        assert st["fullness_after"] <= Rr
        if st["fullness_after"] < 0:
            assert last_qi == 0
    assert abs(total - n * T) <= Rr // 2 + T, (total, n * T)


@pytest.mark.gpu
def test_ffmpeg_in_chromium_plays_a_block_qi_clip(hip, browser):
    """Three qi in key and inter frames (eight modes); each frame FFmpeg shows equals the encoder's reconstruction within
    tests/test_thirdparty_decoder.py's bounds."""
    from tests import test_thirdparty_decoder as tp
    from theora_amd.encoder import ogg_stream
    w, h, n, q, fmt = 64, 48, 6, 36, 0
    frames = M.sequence("shear", w, h, fmt, n, seed=11)
    for fr in frames:
        for p in (1, 2):
            fr[p][:] = 128
    hdr, out = _encode(w, h, fmt, q, frames, 12, inter=True, modes=True, kf=4)
    assert all(o[2]["nqis"] == 3 for o in out if o[0])
    for kind in (True, False):   # key and inter frames both use a second qi; across the clip all three occur
        assert any(sum(o[2]["blocks"][1]) + sum(o[2]["blocks"][2]) for f, o in enumerate(out) if (f % 4 == 0) == kind), kind
    assert all(sum(sum(o[2]["blocks"][k]) for o in out) for k in range(3))
    want = [[o[4][p].astype(np.float64) for p in range(3)] for o in out]
    data = [(o[0], o[1], int(i == n - 1)) for i, o in enumerate(out)]
    res = tp.play(browser, ogg_stream(hdr, data), n)
    assert (res["w"], res["h"]) == (w, h) and len(res["frames"]) == n
    exact = 0
    for f in range(n):
        scores = tp.compare({"frames": [res["frames"][f]] * n}, want, w, h)
        g = min(range(n), key=lambda i: scores[i][0])
        mean, worst_block, share = scores[g]
        assert abs(g - f) <= 1, (f, g)
        assert mean < 0.6 and worst_block < 1.5, (f, g, mean, worst_block)
        exact += g == f
    assert exact >= n - 2


def _sweep(frames, w, h, inter, delta):
    """Per quality 16, 32, 48: (bytes, Y PSNR, the real sum of SSE + lambda bits) of the clip's coded frames of the measured type
    (key frames of an intra-only stream; inter frames with eight modes).  lambda in pixels: the encoder's (s * s * LAM_NUM) >> LAM_SHIFT at the
    frame's qi, over 16 (the fDCT's gain: its coefficients' energy is 16 x the pixels')."""
    from tests.enc_bqi_ref import LAM_NUM, LAM_SHIFT
    from theora_amd.encoder import Encoder
    from theora_amd.decoder import Decoder
    res = []
    for q in (16, 32, 48):
        kw = dict(inter=True, keyframe_interval=64, all_modes=True) if inter else {}
        e = Encoder(w, h, 0, q, block_qi=delta, **kw)
        hdr = e.header_packets()
        setup = enc_ref.SetupParams(hdr[2])
        s = int(setup.qmat(1 if inter else 0, 0, q)[1])
        lam = ((s * s * LAM_NUM) >> LAM_SHIFT) / 16.0
        dec = Decoder(hdr)
        nb, sse, n = 0, 0.0, 0
        for f, fr in enumerate(frames):
            e.encode(fr)
            pkt = e.packetout(f == len(frames) - 1)[0]
            dec.packetin(pkt)
            if inter and f == 0:
                continue
            pic = dec.ycbcr_out()
            nb += len(pkt)
            sse += sum(float(((pic[p].astype(np.float64) - fr[p]) ** 2).sum()) for p in range(3))
            n += 1
        dec.close()
        e.close()
        res.append((nb, 10 * np.log10(255.0 ** 2 * n * w * h * 1.5 / max(sse, 1e-9)), sse + lam * 8 * nb))
    return res


def _bytes_at_matched_psnr(off, on):
    """The on/off byte ratio at the PSNRs both sweeps reach: log-bytes interpolated over PSNR, averaged over the overlap."""
    po, bo = np.array([r[1] for r in off]), np.log(np.array([r[0] for r in off], np.float64))
    pn, bn = np.array([r[1] for r in on]), np.log(np.array([r[0] for r in on], np.float64))
    lo, hi = max(po.min(), pn.min()), min(po.max(), pn.max())
    ps = np.linspace(lo, hi, 16)
    return float(np.exp(np.mean(np.interp(ps, pn, bn) - np.interp(ps, po, bo))))


_GAIN = {}


@pytest.mark.gpu
@pytest.mark.parametrize("inter", [False, True])
def test_block_qi_lowers_the_cost(hip, inter):
    """The natural pan at 352x288 (two key frames of an intra-only stream; three inter frames with eight modes), qualities 16 / 32 /
    48, delta 8: the real SSE + lambda bits falls at every quality, and the bytes at matched PSNR (all three planes) fall by about
    half the measured gain or more (0.965 key, 0.960 inter)."""
    w, h = 352, 288
    frames = IR.sequence("pan", w, h, 0, 2 if not inter else 4, seed=21)
    off, on = _sweep(frames, w, h, inter, 0), _sweep(frames, w, h, inter, 8)
    ratio = _bytes_at_matched_psnr(off, on)
    print("inter" if inter else "key", "off", off, "on", on, "bytes at matched PSNR %.4f" % ratio)
    for (b0, p0, j0), (b1, p1, j1) in zip(off, on):
        assert j1 < j0, (j0, j1)
    assert ratio <= 0.983 if inter else ratio <= 0.982, ratio
