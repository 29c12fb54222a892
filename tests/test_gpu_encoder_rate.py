"""th_encode_* bitrate mode on the GPU: the probe's E[q] equals tests/enc_rate_ref.py's restatement, so do the controller's choices,
drops, fullness, corrections and every packet; the rate holds its target; the streams decode, and the C example's -V agrees."""
import numpy as np
import pytest

import oracle
from tests import enc_inter_ref as R
from tests import enc_rate_ref as RR
from tests import enc_ref
from tests.test_gpu_encoder import _compile, _psnr, _y4m
from tests.test_thirdparty_decoder import browser  # noqa: F401 -- the fixture (skips where that browser cannot run)


def _run(w, h, fmt, frames, bitrate, pic=None, inter=False, kf=12, flags=None, buffer=None, dups=None, retarget=None,
         device_input=False, quality=32, rebuffer=None, recon=False):
    """Headers, and per packet (bytes, granulepos, rate stats) -- with recon, (bytes, granulepos, rate stats, reconstruction)."""
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT, TH_ENCCTL_SET_RATE_BUFFER, Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, inter=inter, keyframe_interval=kf if inter else None, bitrate=bitrate,
                rate_flags=flags, rate_buffer=buffer)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if retarget and f in retarget:
            e.set_bitrate(retarget[f])
        if rebuffer and f in rebuffer:
            assert e.ctl(TH_ENCCTL_SET_RATE_BUFFER, rebuffer[f])[0] == 0
        if dups and dups.get(f):
            assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, dups[f])[0] == 0
        if device_input:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append((r[0], r[1], e.rate_stats()) + ((e.recon(),) if recon else ()))
    e.close()
    return hdr, out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,kind", [
    (64, 48, 0, (1, 2, 61, 45), "natural"), (176, 144, 0, (3, 1, 169, 139), "natural"), (176, 144, 2, None, "noise"),
    (176, 144, 3, None, "natural"), (352, 288, 0, None, "natural"), (352, 288, 2, None, "noise"),
])
def test_key_frame_probe_equals_the_restatement(hip, w, h, fmt, pic, kind):
    p = pic or (0, 0, w, h)
    frame = enc_ref.picture(kind, w, h, fmt, p, seed=w + fmt)
    hdr, out = _run(w, h, fmt, [frame], 10 ** 6, pic=pic)
    setup = enc_ref.SetupParams(hdr[2])
    want = RR.Probe(w, h, fmt, p, setup).key(frame)
    st = out[0][2]
    assert st["key"] == 1 and st["probe"] == [int(x) for x in want]


def _restated(w, h, fmt, frames, hdr, bitrate, inter=False, kf=12, flags=RR.DROP_FRAMES | RR.CAP_OVERFLOW, buffer=None, dups=None,
              retarget=None, rebuffer=None):
    rs = RR.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, inter=inter, kf_interval=kf, flags=flags,
                       buffer=buffer)
    out = []
    try:
        for f, fr in enumerate(frames):
            if retarget and f in retarget:
                rs.ctl.set_bitrate(retarget[f])
            if rebuffer and f in rebuffer:
                rs.ctl.set_buffer(rebuffer[f])
            out.extend(rs.frame(fr, (dups or {}).get(f, 0)))
    finally:
        rs.close()
    return out


def _compare(got, want):
    assert len(got) == len(want)
    for k, ((pkt, gp, st), (wpkt, rec)) in enumerate(zip(got, want)):
        for name, v in rec.items():
            assert st[name] == v, (k, name, st[name], v)
        assert pkt == wpkt, k


@pytest.mark.gpu
def test_inter_probe_equals_the_restatement(hip):
    w, h, fmt = 176, 144, 0
    frames = R.sequence("pan", w, h, fmt, 6, seed=3)
    hdr, got = _run(w, h, fmt, frames, 400000, inter=True, flags=0)
    want = _restated(w, h, fmt, frames, hdr, 400000, inter=True, flags=0)
    assert [g[2]["key"] for g in got] == [1, 0, 0, 0, 0, 0]
    _compare(got, want)


CONTROL = [   # (name, w, h, fmt, inter, bitrate, flags, buffer, dups, retarget, rebuffer)
    ("intra", 96, 64, 0, False, 60000, None, None, None, None, None),
    ("inter", 96, 64, 2, True, 40000, None, None, None, None, None),
    ("inter-noflags", 96, 64, 0, True, 30000, 0, None, None, None, None),
    ("inter-underflow", 96, 64, 0, True, 30000, RR.CAP_UNDERFLOW, 20, None, None, None),
    ("inter-drop-only", 96, 64, 3, True, 15000, RR.DROP_FRAMES, None, None, None, None),
    ("inter-retarget-dups", 96, 64, 0, True, 20000, None, None, {4: 2, 17: 1}, {10: 90000, 20: 12000}, None),
    ("inter-rebuffer", 96, 64, 0, True, 30000, None, None, None, None, {8: 40, 19: 5}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,fmt,inter,bitrate,flags,buffer,dups,retarget,rebuffer", CONTROL, ids=[c[0] for c in CONTROL])
def test_control_equals_the_restatement(hip, name, w, h, fmt, inter, bitrate, flags, buffer, dups, retarget, rebuffer):
    """30 frames: qi, drops, F before and after, c_t, the spend, estimate, probe and every packet equal the restatement; with a
    mid-stream SET_BITRATE, SET_RATE_BUFFER (D, R, F* and F follow) and SET_DUP_COUNT too."""
    frames = R.sequence("pan", w, h, fmt, 30, seed=7)
    hdr, got = _run(w, h, fmt, frames, bitrate, inter=inter, flags=flags, buffer=buffer, dups=dups, retarget=retarget,
                    rebuffer=rebuffer)
    want = _restated(w, h, fmt, frames, hdr, bitrate, inter=inter, flags=RR.DROP_FRAMES | RR.CAP_OVERFLOW if flags is None else flags,
                     buffer=buffer, dups=dups, retarget=retarget, rebuffer=rebuffer)
    if rebuffer:   # the new D shows in the spend: S = F + D T - F*
        f = max(rebuffer)
        st = got[f][2]
        assert st["spend"] == st["fullness_before"] + min(max(rebuffer[f], 12), 256) * st["target"] - \
            min(max(rebuffer[f], 12), 256) * st["target"] // 2
    _compare(got, want)
    print(name, "qi", [g[2]["qi"] for g in got], "dropped", sum(g[2]["dropped"] for g in got))


def _clip_bytes(frames, w, h, q):
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, 0, q, inter=True, keyframe_interval=12)
    e.header_packets()
    n = 0
    for f, fr in enumerate(frames):
        e.encode(fr)
        n += len(e.packetout(f == len(frames) - 1)[0])
    e.close()
    return n


@pytest.mark.gpu
def test_rate_holds_its_target(hip):
    """352x288 pan at 30 fps, 150 frames, D = 12, three targets between the quality-8 and quality-56 streams' rates: F <= R always
    (CAP_OVERFLOW), F < 0 only after a frame coded at qi 0 (DROP_FRAMES), the total within N T +- (R / 2 + T); a higher target gives
    a higher mean qi and a higher mean Y PSNR."""
    from theora_amd.decoder import Decoder
    w, h, n = 352, 288, 150
    frames = R.sequence("pan", w, h, 0, n, seed=21)
    lo, hi = _clip_bytes(frames, w, h, 8) * 8 * 30 // n, _clip_bytes(frames, w, h, 56) * 8 * 30 // n
    means = []
    for bitrate in (lo + (hi - lo) // 6, (lo + hi) // 2, hi - (hi - lo) // 6):
        hdr, out = _run(w, h, 0, frames, bitrate, inter=True, buffer=12)
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
        assert abs(total - n * T) <= Rr // 2 + T, (bitrate, total, n * T)
        dec = Decoder(hdr)
        ps = []
        for f, (pkt, gp, st) in enumerate(out):
            dec.packetin(pkt)
            ps.append(_psnr(dec.ycbcr_out()[0], frames[f][0]))
        dec.close()
        coded = [st["qi"] for _, _, st in out if not st["dropped"]]
        means.append((float(np.mean(coded)), float(np.mean(ps)), sum(st["dropped"] for _, _, st in out)))
    print("quality 8 / 56 rates %d / %d bit/s; (mean qi, mean Y PSNR, drops) per target: %s" % (lo, hi, means))
    assert means[0][0] < means[1][0] < means[2][0]
    assert means[0][1] < means[1][1] < means[2][1]


@pytest.mark.gpu
def test_rate_clip_with_drops_decodes_like_the_oracle(hip):
    """A rate-controlled inter clip with drops: th_decode_*'s pictures equal the restatement's oracle decode frame by frame, and
    host and device input give the same packets."""
    from theora_amd.decoder import Decoder
    w, h, fmt = 96, 64, 0
    frames = R.sequence("cut", w, h, fmt, 20, seed=2)
    hdr, got = _run(w, h, fmt, frames, 15000, inter=True)
    assert sum(g[2]["dropped"] for g in got) >= 1
    _, dev = _run(w, h, fmt, frames, 15000, inter=True, device_input=True)
    assert [g[0] for g in dev] == [g[0] for g in got]
    rs = RR.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 15000, inter=True, kf_interval=12)
    dec = Decoder(hdr)
    try:
        for f, fr in enumerate(frames):
            (wpkt, rec), = rs.frame(fr)
            pkt, gp, st = got[f]
            assert pkt == wpkt and st["dropped"] == rec["dropped"], f
            rc, dgp = dec.packetin(pkt)
            assert dgp == gp
            pic = dec.ycbcr_out()
            for p in range(3):
                assert np.array_equal(pic[p], rs.enc.ost.get_plane(oracle.FRAME_PREV, p)[::-1]), (f, p)
    finally:
        rs.close()
        dec.close()


@pytest.mark.gpu
def test_encoder_example_V_matches_the_python_encoder(hip, tmp_path):
    import subprocess
    from theora_amd.decoder import ogg_packets
    from theora_amd.encoder import Encoder
    w, h, fmt = 96, 64, 0
    frames = R.sequence("pan", w, h, fmt, 14, seed=4)
    exe = _compile(tmp_path, "encoder_example_hip")
    (tmp_path / "in.y4m").write_bytes(_y4m(frames, w, h, "420jpeg"))
    for k in (None, 12):
        args = [exe, "-V", "40"] + (["-k", str(k)] if k else []) + ["-o", str(tmp_path / "out.ogv"), str(tmp_path / "in.y4m")]
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got, (bad, gaps) = ogg_packets((tmp_path / "out.ogv").read_bytes())
        assert (bad, gaps) == (0, 0)
        e = Encoder(w, h, fmt, 48, inter=k is not None, keyframe_interval=k, bitrate=40000)
        want = e.header_packets()
        for f, fr in enumerate(frames):
            e.encode(fr)
            want.append(e.packetout(f == len(frames) - 1)[0])
        e.close()
        assert [g[1] for g in got] == want


@pytest.mark.gpu
def test_ffmpeg_in_chromium_plays_a_rate_clip_with_drops(hip, browser):
    """FFmpeg's Theora decoder in the bundled Chromium plays a bitrate-mode inter clip whose drops are zero-byte packets between coded
    inter frames: each frame shown equals the encoder's reconstruction in force at it (for a drop, the previous frame's) within RGB
    rounding (tests/test_thirdparty_decoder.py's comparison)."""
    from tests import test_thirdparty_decoder as tp
    from theora_amd.encoder import ogg_stream
    w, h, fmt, n = 64, 48, 3, 10
    frames = R.sequence("cut", w, h, fmt, n, seed=11)
    for fr in frames:   # the comparison's colour range: chroma near grey
        for p in (1, 2):
            fr[p][:] = np.clip(128 + (fr[p].astype(np.int64) - 110) // 4, 0, 255)
    hdr, out = _run(w, h, fmt, frames, 12000, inter=True, recon=True)
    dropped = [o[2]["dropped"] for o in out]
    assert len(out) == n and sum(dropped) >= 1 and any(not o[2]["key"] and not d and o[0] for o, d in zip(out, dropped))
    assert all(len(o[0]) == 0 for o, d in zip(out, dropped) if d)
    want = [[o[3][p].astype(np.float64) for p in range(3)] for o in out]
    data = [(o[0], o[1], int(i == n - 1)) for i, o in enumerate(out)]
    res = tp.play(browser, ogg_stream(hdr, data), n)
    assert (res["w"], res["h"]) == (w, h) and len(res["frames"]) == n
    exact = 0
    for f in range(n):
        scores = tp.compare({"frames": [res["frames"][f]] * n}, want, w, h)
        ok = [g for g in range(max(f - 1, 0), min(f + 2, n)) if scores[g][0] < 0.6 and scores[g][1] < 1.5]
        assert ok, (f, dropped, scores)
        exact += f in ok
    assert exact >= n - 2
