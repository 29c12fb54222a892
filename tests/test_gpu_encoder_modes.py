"""th_encode_* with all eight macro-block modes on the GPU (TH_ENCCTL_THIP_SET_INTER_MODES): the packets and mode statistics equal
tests/enc_modes_ref.py's restatement byte for byte, the encoder's reconstruction is th_decode_*'s picture of them, bitrate mode
composes with the switch, and FFmpeg plays the streams."""
import numpy as np
import pytest

from tests import enc_modes_ref as M
from tests import enc_rate_ref as RR
from tests import enc_ref
from tests.test_gpu_encoder_inter import _frames as _inter_frames
from tests.test_thirdparty_decoder import browser  # noqa: F401 -- the fixture (skips where that browser cannot run)


def _frames(kind, w, h, fmt, n, pic):
    if kind not in ("uncover", "shear"):
        return _inter_frames(kind, w, h, fmt, n, pic)
    frames = M.sequence(kind, w, h, fmt, n)
    if pic is None:
        return frames
    return [[a[y0:y0 + ch, x0:x0 + cw] for a, (x0, y0, cw, ch) in zip(fr, [enc_ref.chroma_region(pic, fmt, p) for p in range(3)])]
            for fr in frames]


def _encode(w, h, fmt, quality, frames, pic=None, kf=64, device_input=False):
    """Headers, and per packet (bytes, granulepos, inter stats, mode stats, recon)."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, inter=True, keyframe_interval=kf, all_modes=True)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if device_input:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        r = e.packetout(f == len(frames) - 1)
        out.append((r[0], r[1], e.inter_stats(), e.mode_stats(), e.recon()))
    e.close()
    return hdr, out


CASES = [   # (w, h, fmt, pic, quality, content, key-frame interval, device input, frames)
    (16, 16, 0, None, 32, "pan", 64, False, 4),
    (176, 144, 0, None, 32, "uncover", 64, False, 6),
    (176, 144, 0, None, 24, "shear", 64, True, 4),
    (176, 144, 2, None, 40, "shear", 64, False, 4),
    (176, 144, 3, None, 32, "uncover", 64, True, 6),
    (176, 144, 2, None, 48, "uncover", 4, False, 6),
    (176, 144, 0, None, 48, "cut", 4, True, 6),
    (176, 144, 3, None, 63, "shear", 1, False, 3),
    (176, 144, 0, None, 63, "static", 64, False, 4),
    (64, 48, 0, (1, 2, 61, 45), 32, "pan", 4, False, 6),
    (64, 48, 2, (1, 2, 61, 45), 16, "shear", 64, True, 5),
    (64, 48, 3, (1, 2, 61, 45), 40, "uncover", 64, False, 6),
    (1280, 720, 0, None, 48, "pan", 64, False, 3),
]
_SEEN = np.zeros(8, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,kind,kf,dev,n", CASES)
def test_mode_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, kind, kf, dev, n):
    frames = _frames(kind, w, h, fmt, n, pic)
    hdr, out = _encode(w, h, fmt, quality, frames, pic=pic, kf=kf, device_input=dev)
    ref = M.ModesEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            pkt, gp, st, ms, rec = out[f]
            assert st["key"] == want["key"], f
            assert pkt == want["packet"], (f, len(pkt), len(want["packet"]), ms, want.get("modes8"))
            assert list(ms["modes"].values()) == want["modes8"] and ms["vectors"] == want["vectors"], (f, ms, want["modes8"])
            assert list(st["modes"].values()) == want["modes"] and st["coded"] == want["coded"], (f, st, want["modes"])
            assert (st["mode_scheme"], st["mv_scheme"]) == (want["mode_scheme"], want["mv_scheme"]), f
            for p in range(3):
                assert np.array_equal(rec[p], ref.recon[p]), (f, p)
            if not want["key"]:
                _SEEN[:] += want["modes8"]
    finally:
        ref.close()


@pytest.mark.gpu
def test_all_eight_modes_occur(hip):
    """Across the table above (run first), every mode of the spec is used."""
    if _SEEN.sum() == 0:
        pytest.skip("runs after test_mode_packets_equal_the_restatement")
    assert (_SEEN > 0).all(), _SEEN


@pytest.mark.gpu
@pytest.mark.parametrize("kind,fmt", [("uncover", 0), ("shear", 2)])
def test_recon_is_the_decoders_picture(hip, kind, fmt):
    from theora_amd.decoder import Decoder
    w, h, q = 176, 144, 32
    frames = M.sequence(kind, w, h, fmt, 8, seed=5)
    hdr, out = _encode(w, h, fmt, q, frames)
    dec = Decoder(hdr)
    try:
        for f, (pkt, gp, st, ms, rec) in enumerate(out):
            rc, dgp = dec.packetin(pkt)
            assert dgp == gp
            pic = dec.ycbcr_out()
            for p in range(3):
                assert np.array_equal(rec[p], pic[p]), (f, p)
    finally:
        dec.close()


@pytest.mark.gpu
def test_modes_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_INTER_MODES, Encoder
    e = Encoder(64, 48, 0, 30, inter=True, all_modes=True)
    e.header_packets()
    e.encode(M.sequence("pan", 64, 48, 0, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_INTER_MODES, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_INTER_MODES, 1)[0] == -10
    e.close()


@pytest.mark.gpu
def test_switch_off_counts_five_modes(hip):
    """With the switch off, GET_MODE_STATS is GET_INTER_STATS's five counts and the INTER_MV vectors."""
    from theora_amd.encoder import Encoder
    frames = M.sequence("pan", 176, 144, 0, 4)
    e = Encoder(176, 144, 0, 32, inter=True)
    e.header_packets()
    for f, fr in enumerate(frames):
        e.encode(fr)
        e.packetout(f == 3)
        st, ms = e.inter_stats(), e.mode_stats()
        assert list(ms["modes"].values()) == list(st["modes"].values()) + [0, 0, 0]
        assert ms["vectors"] == st["modes"]["INTER_MV"]
    e.close()


def _rate_run(w, h, fmt, frames, bitrate, kf=12, buffer=None):
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, 32, inter=True, keyframe_interval=kf, bitrate=bitrate, rate_buffer=buffer, all_modes=True)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append((r[0], r[1], e.rate_stats()))
    e.close()
    return hdr, out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,fmt,bitrate", [("shear", 0, 300000), ("uncover", 2, 150000)])
def test_bitrate_mode_equals_the_composed_restatement(hip, kind, fmt, bitrate):
    w, h = 96, 64
    frames = M.sequence(kind, w, h, fmt, 16, seed=7)
    hdr, got = _rate_run(w, h, fmt, frames, bitrate)
    rs = M.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, inter=True, kf_interval=12,
                      flags=RR.DROP_FRAMES | RR.CAP_OVERFLOW)
    want = []
    try:
        for fr in frames:
            want.extend(rs.frame(fr))
    finally:
        rs.close()
    assert len(got) == len(want)
    for k, ((pkt, gp, st), (wpkt, rec)) in enumerate(zip(got, want)):
        for name, v in rec.items():
            assert st[name] == v, (k, name, st[name], v)
        assert pkt == wpkt, k


@pytest.mark.gpu
def test_bitrate_mode_holds_its_target_with_all_modes(hip):
    """test_gpu_encoder_rate.test_rate_holds_its_target's bounds on its pan (middle target) with the switch on."""
    from tests import enc_inter_ref as R
    from tests.test_gpu_encoder_rate import _clip_bytes
    w, h, n = 352, 288, 150
    frames = R.sequence("pan", w, h, 0, n, seed=21)
    lo, hi = _clip_bytes(frames, w, h, 8) * 8 * 30 // n, _clip_bytes(frames, w, h, 56) * 8 * 30 // n
    hdr, out = _rate_run(w, h, 0, frames, (lo + hi) // 2, buffer=12)
    T = out[0][2]["target"]
    Rr = 12 * T
    total, last_qi = 0, None
    for pkt, gp, st in out:
        total += 8 * len(pkt)
        if not st["dropped"] and not st["duplicate"]:
            last_qi = st["qi"]
        assert st["fullness_after"] <= Rr
        if st["fullness_after"] < 0:
            assert last_qi == 0
    assert abs(total - n * T) <= Rr // 2 + T, (total, n * T)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,kind", [(0, "shear"), (3, "uncover")])
def test_ffmpeg_in_chromium_plays_an_eight_mode_clip(hip, browser, fmt, kind):
    """4:2:0 shear exercises INTER_MV_FOUR's averaged chroma vector; 4:4:4 uncover the golden modes.  Each frame FFmpeg shows
    equals the encoder's reconstruction within tests/test_thirdparty_decoder.py's bounds."""
    from tests import test_thirdparty_decoder as tp
    from theora_amd.encoder import ogg_stream
    w, h, n, q = 64, 48, 6, 40
    frames = M.sequence(kind, w, h, fmt, n, seed=11)
    for fr in frames:   # the comparison's colour range: chroma near grey (4:2:0: grey, as subsampled chroma compares where flat)
        for p in (1, 2):
            fr[p][:] = 128 if fmt == 0 else np.clip(128 + (fr[p].astype(np.int64) - 110) // 4, 0, 255)
    hdr, out = _encode(w, h, fmt, q, frames)
    used = np.sum([list(o[3]["modes"].values()) for o in out[1:]], 0)
    assert used[M.MV_FOUR if kind == "shear" else M.GOLDEN_NOMV] + (used[M.GOLDEN_MV] if kind == "uncover" else 0) > 0, used
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
