"""th_encode_* with inter frames on the GPU: the packets equal tests/enc_inter_ref.py's restatement byte for byte, the encoder's
reconstruction is the picture both th_decode_* and the oracle make of them (no drift), granules and duplicates stay straight across
key frames, the stream is far smaller than the all-key one on moving content at a like PSNR, and other players read it."""
import numpy as np
import pytest

from tests import enc_inter_ref as R
from tests import enc_ref
from tests.test_gpu_encoder import _compile, _psnr, _y4m
from tests.test_thirdparty_decoder import browser  # noqa: F401 -- the fixture (skips where that browser cannot run)


def _encode(w, h, fmt, quality, frames, pic=None, kf=None, device_input=False, kfgshift=6, dups=None, inter=True):
    """Headers, and per packet (bytes, granulepos, inter stats, recon or None) of encoding `frames`."""
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT, Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, kfgshift=kfgshift, inter=inter, keyframe_interval=kf if inter else None)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if dups and dups[f]:
            assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, dups[f])[0] == 0
        if device_input:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        first = True
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append((r[0], r[1], e.inter_stats(), e.recon() if inter and first else None))
            first = False
    e.close()
    return hdr, out


CASES = [   # (w, h, fmt, pic, quality, content, key-frame interval, device input, frames)
    (16, 16, 0, None, 32, "pan", 64, False, 4),
    (176, 144, 0, None, 16, "pan", 64, False, 6),
    (176, 144, 0, None, 48, "cut", 4, True, 6),
    (176, 144, 2, None, 0, "pan", 64, True, 4),
    (176, 144, 3, None, 63, "pan", 1, False, 3),
    (176, 144, 0, None, 63, "static", 64, False, 5),
    (176, 144, 3, None, 32, "cut", 64, True, 6),
    (64, 48, 0, (1, 2, 61, 45), 32, "pan", 4, False, 6),
    (64, 48, 2, (1, 2, 61, 45), 48, "cut", 64, True, 5),
    (64, 48, 3, (1, 2, 61, 45), 16, "static", 64, False, 4),
    (1280, 720, 0, None, 48, "pan", 64, False, 3),
]


def _frames(kind, w, h, fmt, n, pic):
    frames = R.sequence(kind, w, h, fmt, n)
    if pic is None:
        return frames
    # picture-size input: the crop of the frame-size sequence
    return [[a[y0:y0 + ch, x0:x0 + cw] for a, (x0, y0, cw, ch) in zip(fr, [enc_ref.chroma_region(pic, fmt, p) for p in range(3)])]
            for fr in frames]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,kind,kf,dev,n", CASES)
def test_inter_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, kind, kf, dev, n):
    frames = _frames(kind, w, h, fmt, n, pic)
    hdr, out = _encode(w, h, fmt, quality, frames, pic=pic, kf=kf, device_input=dev)
    ref = R.InterEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            pkt, gp, st, rec = out[f]
            assert st["key"] == want["key"], f
            assert pkt == want["packet"], (f, len(pkt), len(want["packet"]), st)
            assert list(st["modes"].values()) == want["modes"] and st["coded"] == want["coded"], (f, st, want["modes"])
            assert (st["mode_scheme"], st["mv_scheme"]) == (want["mode_scheme"], want["mv_scheme"]), f
            for p in range(3):
                assert np.array_equal(rec[p], ref.recon[p]), (f, p)
    finally:
        ref.close()
    if kind == "cut" and w >= 176:
        assert any(o[2]["modes"]["INTRA"] for o in out[1:] if not o[2]["key"])
    if kind == "static":
        assert any(not o[2]["key"] and sum(o[2]["coded"]) < sum(out[0][2]["coded"]) for o in out)


@pytest.mark.gpu
def test_host_and_device_input_give_the_same_packets(hip):
    frames = R.sequence("cut", 176, 144, 0, 6, seed=3)
    a = _encode(176, 144, 0, 40, frames, kf=4)
    b = _encode(176, 144, 0, 40, frames, kf=4, device_input=True)
    assert [o[0] for o in a[1]] == [o[0] for o in b[1]]


@pytest.mark.gpu
def test_reconstruction_does_not_drift(hip):
    """30 frames at 176x144: every frame's Encoder.recon() is th_decode_*'s picture on the GPU and the oracle's decode of the
    restatement's coded lists, modes and vectors."""
    from theora_amd.decoder import Decoder
    w, h, fmt, q = 176, 144, 0, 32
    frames = R.sequence("pan", w, h, fmt, 30, seed=5)
    hdr, out = _encode(w, h, fmt, q, frames)
    assert sum(o[2]["key"] for o in out) == 1
    dec = Decoder(hdr)
    ref = R.InterEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
    try:
        for f, (pkt, gp, st, rec) in enumerate(out):
            want = ref.frame(frames[f], q)
            assert pkt == want["packet"], f
            rc, dgp = dec.packetin(pkt)
            assert dgp == gp
            pic = dec.ycbcr_out()
            for p in range(3):
                assert np.array_equal(rec[p], pic[p]), (f, p)
                assert np.array_equal(rec[p], ref.recon[p]), (f, p)
    finally:
        ref.close()
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 3, 6])
def test_inter_granules_and_duplicates(hip, shift):
    """Duplicates across a key-frame boundary: the granules are what the decoder reports, duplicates never reach the key-frame
    field, and a frame whose duplicates would is a key frame."""
    from theora_amd.decoder import Decoder
    w, h, fmt = 64, 48, 0
    frames = R.sequence("pan", w, h, fmt, 9, seed=2)
    dups = [0, 1, 0, 2, 1, 0, 1, 0, 3]
    hdr, out = _encode(w, h, fmt, 40, frames, kfgshift=shift, dups=dups)   # (the default interval, 1 << shift)
    assert len(out) == 9 + sum(dups)
    dec = Decoder(hdr)
    key = cur = -1
    keys = []
    for pkt, gp, st, rec in out:
        rc, dgp = dec.packetin(pkt)
        assert gp == dgp
        cur += 1
        if rec is not None:   # (a frame, not a duplicate)
            keys.append(st["key"])
            key = cur if st["key"] else key
        if shift:
            assert 0 <= cur - key < (1 << shift) and gp == ((key + 1) << shift) + (cur - key)
    dec.close()
    if shift == 0:
        assert all(keys)
    elif shift == 3:   # frames 4 and 8 sit at offsets 7 and 5 with 1 and 3 duplicates: they would reach 8, so they are key frames
        assert keys == [True, False, False, False, True, False, False, False, True]
    else:
        assert keys == [True] + [False] * 8


@pytest.mark.gpu
def test_inter_frames_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_INTER_FRAMES, Encoder
    e = Encoder(64, 48, 0, 30, inter=True)
    e.header_packets()
    e.encode(R.sequence("pan", 64, 48, 0, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_INTER_FRAMES, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == -10
    e.close()


def _stream_numbers(frames, w, h, fmt, q, inter):
    from theora_amd.decoder import Decoder
    hdr, out = _encode(w, h, fmt, q, frames, inter=inter)
    dec = Decoder(hdr)
    psnr = []
    for f, o in enumerate(out):
        dec.packetin(o[0])
        psnr.append(_psnr(dec.ycbcr_out()[0], frames[f][0]))
    dec.close()
    return sum(len(o[0]) for o in out), psnr


@pytest.mark.gpu
def test_inter_stream_is_smaller_at_a_like_psnr(hip):
    """A panning natural sequence at quality 32: well under the all-key stream's bytes, no frame's Y PSNR more than 1 dB below the
    all-key one's; noise: at most 5 % more bytes.  Measured: 0.535 of the bytes at +0.6..+1.3 dB -- the
    inter tables of the setup header are finer than the intra ones, so inter frames also refine the reference."""
    w, h, fmt, q = 352, 288, 0, 32
    pan = R.sequence("pan", w, h, fmt, 10, seed=9)
    bi, pi = _stream_numbers(pan, w, h, fmt, q, True)
    bk, pk = _stream_numbers(pan, w, h, fmt, q, False)
    noise = [[enc_ref.content("noise", s, 100 + 3 * f + p) for p, s in enumerate([(h, w), (h // 2, w // 2), (h // 2, w // 2)])]
             for f in range(6)]
    ni, _ = _stream_numbers(noise, w, h, fmt, q, True)
    nk, _ = _stream_numbers(noise, w, h, fmt, q, False)
    print("pan: inter %d bytes, all-key %d bytes (%.3f); Y PSNR inter %s, key %s" % (bi, bk, bi / bk, np.round(pi, 2), np.round(pk, 2)))
    print("noise: inter %d bytes, all-key %d bytes (%.4f)" % (ni, nk, ni / nk))
    assert bi <= 0.6 * bk
    assert all(a >= b - 1.0 for a, b in zip(pi, pk))
    assert ni <= 1.05 * nk


@pytest.mark.gpu
def test_encoder_example_k_matches_the_python_encoder(hip, tmp_path):
    import subprocess
    from theora_amd.decoder import ogg_packets
    from theora_amd.encoder import Encoder
    w, h, fmt = 170, 138, 0
    fw, fh = (w + 15) & ~15, (h + 15) & ~15
    pic = (0, 0, w, h)
    frames = _frames("cut", fw, fh, fmt, 12, pic)
    exe = _compile(tmp_path, "encoder_example_hip")
    (tmp_path / "in.y4m").write_bytes(_y4m(frames, w, h, "420jpeg"))
    for k in (None, 8):
        args = [exe, "-q", "40"] + (["-k", str(k)] if k else []) + ["-o", str(tmp_path / "out.ogv"), str(tmp_path / "in.y4m")]
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got, (bad, gaps) = ogg_packets((tmp_path / "out.ogv").read_bytes())
        assert (bad, gaps) == (0, 0)
        e = Encoder(fw, fh, fmt, 40, pic=pic, inter=k is not None, keyframe_interval=k)
        want = e.header_packets()
        keys = []
        for f, fr in enumerate(frames):
            e.encode(fr)
            want.append(e.packetout(f == len(frames) - 1)[0])
            keys.append(e.inter_stats()["key"])
        e.close()
        assert [g[1] for g in got] == want
        assert keys == ([True] * 12 if k is None else [f % 8 == 0 for f in range(12)])


@pytest.mark.gpu
def test_ffmpeg_in_chromium_plays_an_inter_clip(hip, browser):
    """FFmpeg's Theora decoder in the bundled Chromium plays an inter clip; its frames equal the encoder's reconstruction within RGB
    rounding (tests/test_thirdparty_decoder.py's comparison)."""
    from tests import test_thirdparty_decoder as tp
    from theora_amd.encoder import ogg_stream
    w, h, fmt, n, q = 64, 48, 3, 6, 40
    frames = R.sequence("pan", w, h, fmt, n, seed=11)
    for fr in frames:   # the comparison's colour range: chroma near grey
        for p in (1, 2):
            fr[p][:] = np.clip(128 + (fr[p].astype(np.int64) - 110) // 4, 0, 255)
    hdr, out = _encode(w, h, fmt, q, frames)
    assert sum(not o[2]["key"] for o in out) == n - 1
    want = [[o[3][p].astype(np.float64) for p in range(3)] for o in out]
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
