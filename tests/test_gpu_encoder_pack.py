"""th_encode_*'s device packetiser (TH_ENCCTL_THIP_SET_DEVICE_PACK) on the GPU: the packets equal the restatements byte for byte
(tests/enc_ref.py, enc_inter_ref.py, enc_modes_ref.py, enc_bqi_ref.py -- which know nothing of the packetiser), everything that
follows from a packet equals what the host packer gives, and the edges of the three steps -- EOB runs longer than 4095 and across
lists, every bit phase the frame header can leave, dense and empty packets, the fall-back -- are met on purpose."""
import numpy as np
import pytest

from tests import enc_bqi_ref as B
from tests import enc_inter_ref as R
from tests import enc_modes_ref as M
from tests import enc_ref
from tests.test_gpu_encoder import CASES as KEY_CASES
from tests.test_gpu_encoder_bqi import CASES as BQI_CASES
from tests.test_gpu_encoder_inter import CASES as INTER_CASES
from tests.test_gpu_encoder_modes import CASES as MODES_CASES
from tests.test_thirdparty_decoder import browser  # noqa: F401 -- the fixture (skips where that browser cannot run)


def _crop(frames, fmt, pic):
    if pic is None:
        return frames
    reg = [enc_ref.chroma_region(pic, fmt, p) for p in range(3)]
    return [[a[y0:y0 + ch, x0:x0 + cw] for a, (x0, y0, cw, ch) in zip(fr, reg)] for fr in frames]


def _frames(kind, w, h, fmt, n, pic, seed=0):
    seq = M.sequence if kind in ("uncover", "shear") else R.sequence
    return _crop(seq(kind, w, h, fmt, n, seed=seed), fmt, pic)


def _run(w, h, fmt, quality, frames, pack, pic=None, device_input=False, flip=None, recon=True, **kw):
    """Headers, and per frame a dict of the packet and every statistic, with the packetiser on (pack) or off; flip: a function of the
    frame number that says what the setting is from that frame on (TH_ENCCTL_THIP_SET_DEVICE_PACK between frames)."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, device_pack=pack, **kw)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if flip is not None:
            e.set_device_pack(flip(f))
        if device_input:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        r = e.packetout(f == len(frames) - 1)
        out.append(dict(packet=r[0], gp=r[1], stats=e.stats(), inter=e.inter_stats(), modes=e.mode_stats(), bqi=e.block_qi_stats(),
                        pack=e.pack_stats(), rate=e.rate_stats() if e.bitrate else None,
                        recon=e.recon() if recon and kw.get("inter") else None))
    e.close()
    return hdr, out


def _packed_on_device(out):
    """Every non-empty packet came from the packetiser, and its statistics describe it."""
    for f, o in enumerate(out):
        ps = o["pack"]
        if not o["packet"]:
            assert ps["device"] == 0 and ps["token_bits"] == 0, (f, ps)
            continue
        assert ps["device"] == 1 and ps["fallbacks"] == 0, (f, ps)
        assert ps["phase"] == ps["header_bits"] % 8 and (ps["header_bits"] + ps["token_bits"] + 7) // 8 == len(o["packet"]), (f, ps)
        assert ps["pack_ms"] > 0


# ---- byte equality with the restatements ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,kind", [c for c in KEY_CASES if c[0] * c[1] <= 1280 * 720])
def test_key_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, kind):
    p = pic or (0, 0, w, h)
    frame = enc_ref.picture(kind, w, h, fmt, p, seed=w + quality)
    hdr, out = _run(w, h, fmt, quality, [frame], True, pic=pic)
    ref = enc_ref.encode_frame(frame, w, h, fmt, p, quality, enc_ref.SetupParams(hdr[2]))
    st = out[0]["stats"]
    assert (st["tokens"], st["tokens_merged"], st["huff"], st["overflow"]) == (ref["tokens"], ref["tokens_merged"], ref["huff"], 0)
    assert out[0]["packet"] == ref["packet"]
    _packed_on_device(out)
    assert out[0]["pack"]["phase"] == 4 and out[0]["pack"]["header_bits"] == 12   # a plain key frame's header
    dev = _run(w, h, fmt, quality, [frame], True, pic=pic, device_input=True)[1]
    assert dev[0]["packet"] == ref["packet"] and dev[0]["pack"]["device"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,kind,kf,dev,n", [c for c in INTER_CASES if c[0] <= 176])
def test_inter_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, kind, kf, dev, n):
    frames = _frames(kind, w, h, fmt, n, pic)
    hdr, out = _run(w, h, fmt, quality, frames, True, pic=pic, device_input=dev, inter=True, keyframe_interval=kf)
    ref = R.InterEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            assert out[f]["packet"] == want["packet"], (f, len(out[f]["packet"]), len(want["packet"]), out[f]["pack"])
            for p in range(3):
                assert np.array_equal(out[f]["recon"][p], ref.recon[p]), (f, p)
    finally:
        ref.close()
    _packed_on_device(out)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,kind,kf,dev,n", [c for c in MODES_CASES if c[0] <= 176])
def test_mode_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, kind, kf, dev, n):
    frames = _frames(kind, w, h, fmt, n, pic)
    hdr, out = _run(w, h, fmt, quality, frames, True, pic=pic, device_input=dev, inter=True, keyframe_interval=kf, all_modes=True)
    ref = M.ModesEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            assert out[f]["packet"] == want["packet"], (f, len(out[f]["packet"]), len(want["packet"]), out[f]["pack"])
            assert list(out[f]["modes"]["modes"].values()) == want["modes8"], f
    finally:
        ref.close()
    _packed_on_device(out)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,delta,kind,inter,modes,dev,n", BQI_CASES)
def test_bqi_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, delta, kind, inter, modes, dev, n):
    frames = _crop(M.sequence(kind, w, h, fmt, n, seed=0), fmt, pic)
    kf = 4 if inter else 1
    kw = dict(inter=True, keyframe_interval=kf, all_modes=modes) if inter else {}
    hdr, out = _run(w, h, fmt, quality, frames, True, pic=pic, device_input=dev, block_qi=delta, **kw)
    ref = B.BqiEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6, delta, modes=modes)
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, quality)
            assert out[f]["bqi"] == want["bqi"], (f, out[f]["bqi"], want["bqi"])
            assert out[f]["packet"] == want["packet"], (f, len(out[f]["packet"]), len(want["packet"]), out[f]["pack"])
            if inter:   # th_decode_*'s picture of the packets is the oracle's
                for p in range(3):
                    assert np.array_equal(out[f]["recon"][p], ref.recon[p]), (f, p)
    finally:
        ref.close()
    _packed_on_device(out)


# ---- on equals off ----------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    """Two runs agree in everything but the packetiser's own statistics and the timing fields of the rate statistics."""
    assert a[0] == b[0], what   # headers
    assert len(a[1]) == len(b[1])
    for f, (x, y) in enumerate(zip(a[1], b[1])):
        for k in ("packet", "gp", "stats", "inter", "modes", "bqi"):
            assert x[k] == y[k], (what, f, k, x[k] if k != "packet" else len(x[k]), y[k] if k != "packet" else len(y[k]))
        if x["rate"] is not None:
            drop = ("probe_ms", "control_ms")
            assert {k: v for k, v in x["rate"].items() if k not in drop} == {k: v for k, v in y["rate"].items() if k not in drop}, (what, f)
        if x["recon"] is not None:
            for p in range(3):
                assert np.array_equal(x["recon"][p], y["recon"][p]), (what, f, p)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(inter=True, keyframe_interval=5), dict(inter=True, keyframe_interval=5, all_modes=True),
                                dict(inter=True, keyframe_interval=4, all_modes=True, block_qi=8), dict(block_qi=6)],
                         ids=["key", "inter", "modes", "modes-bqi", "key-bqi"])
def test_on_equals_off_and_flipped(hip, kw):
    w, h, fmt, n = 176, 144, 0, 9
    frames = M.sequence("shear", w, h, fmt, n, seed=7)
    off = _run(w, h, fmt, 36, frames, False, **kw)
    on = _run(w, h, fmt, 36, frames, True, **kw)
    assert all(o["pack"]["device"] == 0 and o["pack"]["pack_ms"] == 0 for o in off[1])
    _packed_on_device(on[1])
    _same(off, on, "on")
    flipped = _run(w, h, fmt, 36, frames, False, flip=lambda f: f % 3 != 1, **kw)
    assert [o["pack"]["device"] for o in flipped[1] if o["packet"]] == [int(f % 3 != 1) for f, o in enumerate(flipped[1]) if o["packet"]]
    _same(off, flipped, "flipped")


@pytest.mark.gpu
@pytest.mark.parametrize("kw,bitrate", [(dict(inter=True, keyframe_interval=6), 600000), (dict(), 2500000),
                                        (dict(inter=True, keyframe_interval=6, all_modes=True, block_qi=8), 400000)],
                         ids=["inter", "key", "modes-bqi"])
def test_on_equals_off_in_bitrate_mode(hip, kw, bitrate):
    """A and the block-qi tables feed back into later frames: equal qi choices, drops, and rate statistics."""
    w, h, fmt, n = 176, 144, 0, 14
    frames = M.sequence("uncover", w, h, fmt, n, seed=2)
    off = _run(w, h, fmt, 32, frames, False, bitrate=bitrate, **kw)
    on = _run(w, h, fmt, 32, frames, True, bitrate=bitrate, **kw)
    _same(off, on, "rate")
    assert any(o["rate"]["corr"] != [65536, 65536] for o in on[1])   # (packet sizes did feed back into the controller)
    _packed_on_device([o for o in on[1] if not o["rate"]["dropped"]])


@pytest.mark.gpu
def test_setting_refused_between_in_and_out(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_DEVICE_PACK, Encoder
    frame = enc_ref.picture("natural", 64, 48, 0, (0, 0, 64, 48), seed=1)
    e = Encoder(64, 48, 0, 30)
    e.header_packets()
    e.encode(frame)
    assert e.ctl(TH_ENCCTL_THIP_SET_DEVICE_PACK, 1)[0] == -10
    a = e.packetout()[0]
    assert e.pack_stats()["device"] == 0
    assert e.ctl(TH_ENCCTL_THIP_SET_DEVICE_PACK, 1)[0] == 0
    e.encode(frame)
    b = e.packetout()[0]
    assert e.pack_stats()["device"] == 1 and a == b
    e.close()


# ---- EOB-run edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,blocks,pieces", [(512, 256, 2, 4096, 2), (704, 576, 0, 9504, 3)])
@pytest.mark.parametrize("textured", [False, True])
@pytest.mark.parametrize("quality", [0, 32, 63])
def test_eob_runs_beyond_4095(hip, w, h, fmt, blocks, pieces, textured, quality):
    """Planes of 128 throughout: every block is one EOB at index 0 and the frame one run of `blocks`, cut into pieces of 4095 from its
    start.  With one textured macro block in the middle the runs end and start again in every list the macro block has tokens in."""
    frame = [np.full(s, 128, np.uint8) for s in enc_ref.plane_shapes(w, h, fmt)]
    if textured:
        rng = np.random.default_rng(5)
        hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
        y0, x0 = (h // 32) * 16, (w // 32) * 16
        frame[0][y0:y0 + 16, x0:x0 + 16] = rng.integers(0, 256, (16, 16), dtype=np.uint8)
        for p in (1, 2):
            frame[p][y0 >> vd:(y0 + 16) >> vd, x0 >> hd:(x0 + 16) >> hd] = rng.integers(0, 256, (16 >> vd, 16 >> hd), dtype=np.uint8)
    hdr, out = _run(w, h, fmt, quality, [frame], True)
    ref = enc_ref.encode_frame(frame, w, h, fmt, (0, 0, w, h), quality, enc_ref.SetupParams(hdr[2]))
    if not textured:   # the intended pieces occur: 4095 + 1, and 4095 + 4095 + 1314
        assert (ref["tokens"], ref["tokens_merged"]) == (blocks, pieces)
        assert len(ref["packet"]) == (6 if pieces == 2 else 10)
    else:              # ... and here more runs than that, over more tokens than blocks
        assert ref["tokens"] > blocks and pieces < ref["tokens_merged"] < ref["tokens"]
    st = out[0]["stats"]
    assert (st["tokens"], st["tokens_merged"], st["huff"]) == (ref["tokens"], ref["tokens_merged"], ref["huff"])
    assert out[0]["packet"] == ref["packet"]
    _packed_on_device(out)


# ---- the header's bit phase -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_every_phase_of_the_header(hip):
    """The header of an inter frame ends at any bit: over these clips at least six of the eight phases occur, all byte-equal."""
    seen = set()
    for k, (kind, quality, fmt, modes) in enumerate([("pan", 20, 0, False), ("cut", 44, 2, False), ("shear", 32, 0, True),
                                                      ("uncover", 52, 3, True), ("pan", 60, 2, True)]):
        w, h, n = 96, 64, 8
        frames = _frames(kind, w, h, fmt, n, None, seed=20 + k)
        hdr, out = _run(w, h, fmt, quality, frames, True, inter=True, keyframe_interval=64, all_modes=modes, recon=False)
        ref = (M.ModesEncoder if modes else R.InterEncoder)(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
        try:
            for f, fr in enumerate(frames):
                assert out[f]["packet"] == ref.frame(fr, quality)["packet"], (k, f, out[f]["pack"])
        finally:
            ref.close()
        _packed_on_device(out)
        assert out[0]["pack"]["phase"] == 4
        seen |= {o["pack"]["phase"] for o in out[1:] if o["packet"]}
    assert len(seen) >= 6, seen


# ---- dense and empty ends ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dense_noise_at_quality_63(hip):
    w, h = 352, 288
    frame = enc_ref.picture("noise", w, h, 0, (0, 0, w, h), seed=9)
    hdr, out = _run(w, h, 0, 63, [frame], True)
    ref = enc_ref.encode_frame(frame, w, h, 0, (0, 0, w, h), 63, enc_ref.SetupParams(hdr[2]))
    assert ref["tokens"] > 40 * (w * h * 3 // 2 // 64)   # dense: most coefficients have a token of their own
    assert out[0]["packet"] == ref["packet"]
    _packed_on_device(out)


@pytest.mark.gpu
def test_still_clip_gives_empty_packets(hip):
    w, h = 64, 48
    frame = [np.full(s, 128, np.uint8) for s in enc_ref.plane_shapes(w, h, 0)]   # (the reconstruction is exact: nothing left to code)
    off = _run(w, h, 0, 40, [frame] * 4, False, inter=True, keyframe_interval=64)
    on = _run(w, h, 0, 40, [frame] * 4, True, inter=True, keyframe_interval=64)
    _same(off, on, "still")
    assert on[1][0]["packet"] and all(not o["packet"] for o in on[1][1:])
    _packed_on_device(on[1])


@pytest.mark.gpu
def test_one_macro_block(hip):
    frame = enc_ref.picture("noise", 16, 16, 0, (0, 0, 16, 16), seed=3)
    for q in (0, 40, 63):
        hdr, out = _run(16, 16, 0, q, [frame], True)
        assert out[0]["packet"] == enc_ref.encode_frame(frame, 16, 16, 0, (0, 0, 16, 16), q, enc_ref.SetupParams(hdr[2]))["packet"]
        _packed_on_device(out)


# ---- the fall-back ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fall_back_to_the_host_packer(hip):
    """With the device's packet buffer forced small the host packs the frame: the same packet, device 0, and counted."""
    from theora_amd import _lib
    L = _lib.load()
    w, h = 176, 144
    frames = R.sequence("pan", w, h, 0, 4, seed=1)
    want = _run(w, h, 0, 40, frames, False, inter=True, keyframe_interval=64)
    before = L.thip_option(b"enc_pack_cap")
    try:
        assert L.thip_set_option(b"enc_pack_cap", 256) == 0
        got = _run(w, h, 0, 40, frames, True, inter=True, keyframe_interval=64)
    finally:
        L.thip_set_option(b"enc_pack_cap", before)
    _same(want, got, "fall-back")
    assert sum(len(o["packet"]) > 400 for o in got[1]) >= 2
    count = 0
    for o in got[1]:   # (256 bytes bound the device's bytes, which are the packet's less its header's whole bytes)
        if not o["packet"]:
            continue
        count += o["pack"]["device"] == 0
        assert o["pack"]["fallbacks"] == count, o["pack"]
        assert o["pack"]["device"] == 0 or len(o["packet"]) < 400, o["pack"]
        assert o["pack"]["device"] == 1 or len(o["packet"]) > 200, o["pack"]
    assert count >= 2


# ---- another decoder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ffmpeg_in_chromium_plays_a_device_packed_clip(hip, browser):
    """Key and inter frames (eight modes) packed on the device; each frame FFmpeg shows equals the encoder's reconstruction within
    tests/test_thirdparty_decoder.py's bounds."""
    from tests import test_thirdparty_decoder as tp
    from theora_amd.encoder import ogg_stream
    w, h, n, q, fmt = 64, 48, 6, 36, 0
    frames = M.sequence("shear", w, h, fmt, n, seed=11)
    for fr in frames:
        for p in (1, 2):
            fr[p][:] = 128
    hdr, out = _run(w, h, fmt, q, frames, True, inter=True, keyframe_interval=4, all_modes=True)
    _packed_on_device(out)
    want = [[o["recon"][p].astype(np.float64) for p in range(3)] for o in out]
    data = [(o["packet"], o["gp"], int(i == n - 1)) for i, o in enumerate(out)]
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
