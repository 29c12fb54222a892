"""th_encode_* with automatic key frames on the GPU (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES): every packet, granule, inter statistic,
cut statistic (measured, cut, P, I, N) and reconstruction equals tests/enc_cut_ref.py's restatement exactly -- in quality mode with five
and eight modes, block qi and the device packetiser, and in bitrate mode with the controller's record too; content that never cuts gives
the packets of the switch off byte for byte (the test of k_enc_mb_modes and of the probe on the shared statistics); a decoder can
start at the cut key frame; the reference decoder takes the stream."""
import functools

import numpy as np
import pytest

from tests import enc_cut_ref as CR
from tests import enc_ref

T = CR.RECOMMENDED
CUT_FIELDS = ("measured", "cut", "pred", "intra", "intra_mbs", "ratio")
RATE_TIMES = ("probe_ms", "control_ms")


def _crop(frames, fmt, pic):
    if pic is None:
        return frames
    reg = [enc_ref.chroma_region(pic, fmt, p) for p in range(3)]
    return [[np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in zip(fr, reg)] for fr in frames]


def _encode(w, h, fmt, quality, frames, t=T, pic=None, kf=64, dev=False, modes=False, bqi=0, pack=None, dups=None, bitrate=None):
    """Headers, and per packet a dict: pkt, gp, inter (statistics), cut (statistics), recon (a frame's own packet only), rate."""
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT, Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, inter=True, keyframe_interval=kf, all_modes=modes, block_qi=bqi, device_pack=pack,
                bitrate=bitrate, auto_keyframes=t)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if dups and dups.get(f):
            assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, dups[f])[0] == 0
        if dev:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        first = True
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], gp=r[1], inter=e.inter_stats(), cut=e.cut_stats(), recon=e.recon() if first else None,
                            rate=e.rate_stats() if bitrate else None, bqi=e.block_qi_stats() if bqi else None,
                            pack=e.pack_stats() if pack else None))
            first = False
    e.close()
    return hdr, out


def _check(w, h, fmt, quality, frames, hdr, got, cuts, pic=None, kf=64, modes=False, bqi=0, dups=None):
    """got against the restatement, frame by frame (duplicates too); cuts: the frames the restatement must make cut key frames."""
    ref = CR.encoder(T, w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6, modes=modes, bqi=bqi)
    k, seen = 0, []
    try:
        for f, fr in enumerate(frames):
            nd = (dups or {}).get(f, 0)
            want = ref.frame(fr, quality, dups=nd)
            g = got[k]
            assert {n: g["cut"][n] for n in CUT_FIELDS} == {n: want["cut"][n] for n in CUT_FIELDS}, (f, g["cut"], want["cut"])
            assert g["cut"]["measure_ms"] > 0 if want["cut"]["measured"] else g["cut"]["measure_ms"] == 0
            assert g["inter"]["key"] == want["key"], f
            assert g["pkt"] == want["packet"], (f, len(g["pkt"]), len(want["packet"]))
            assert g["gp"] == ((ref.key + 1) << 6) + (ref.cur - nd - ref.key), (f, g["gp"])
            assert list(g["inter"]["modes"].values()) == want["modes"] and g["inter"]["coded"] == want["coded"], f
            assert (g["inter"]["mode_scheme"], g["inter"]["mv_scheme"]) == (want["mode_scheme"], want["mv_scheme"]), f
            if bqi:
                assert g["bqi"] == want["bqi"], f
            for p in range(3):
                assert np.array_equal(g["recon"][p], ref.recon[p]), (f, p)
            if want["cut"]["cut"]:
                seen.append(f)
            for d in range(nd):   # a duplicate: an empty packet, the next granule, nothing measured
                g = got[k + 1 + d]
                assert g["pkt"] == b"" and g["gp"] == ((ref.key + 1) << 6) + (ref.cur - nd - ref.key) + 1 + d
                assert {n: g["cut"][n] for n in CUT_FIELDS} == dict(CR.NO_STATS, ratio=T) and g["cut"]["measure_ms"] == 0
            k += 1 + nd
        assert k == len(got) and seen == cuts, (seen, cuts)
    finally:
        ref.close()


QUALITY_CASES = [   # (name, w, h, fmt, pic, quality, clip, frames, cut at, interval, device input, switches, the cut key frames)
    ("one_macro_block", 16, 16, 0, None, 32, "scene", 4, 2, 64, False, {}, [2]),
    ("less_than_a_wave_422_cropped_device_input", 64, 48, 2, (1, 2, 61, 45), 32, "scene", 5, 2, 64, True, {}, [2]),
    ("444", 176, 144, 3, None, 32, "scene", 5, 2, 64, False, {}, [2]),
    ("two_work_groups", 352, 288, 0, None, 32, "scene", 4, 2, 64, False, {}, [2]),
    ("interval_4", 176, 144, 0, None, 32, "scene", 9, 3, 4, False, {}, [3]),
    ("eight_modes", 176, 144, 0, None, 32, "scene", 6, 3, 64, False, dict(modes=True), [3]),
    ("block_qi", 176, 144, 0, None, 32, "scene", 5, 2, 64, False, dict(bqi=8), [2]),
    ("device_pack", 176, 144, 0, None, 32, "scene", 5, 2, 64, True, dict(pack=True), [2]),
] + [("qcif_%s_q%d" % (kind, q), 176, 144, 0, None, q, kind, n, 3, 64, False, {}, cuts)
     for q in (16, 48) for kind, n, cuts in (("scene", 6, [3]), ("cut", 6, [3, 4, 5]), ("pan", 4, []), ("static", 4, []), ("flat_noise", 4, []))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,fmt,pic,quality,kind,n,cut,kf,dev,sw,cuts", QUALITY_CASES, ids=[c[0] for c in QUALITY_CASES])
def test_cut_packets_equal_the_restatement(hip, name, w, h, fmt, pic, quality, kind, n, cut, kf, dev, sw, cuts):
    frames = _crop(CR.clip(kind, w, h, fmt, n, seed=0, cut=cut), fmt, pic)
    hdr, got = _encode(w, h, fmt, quality, frames, pic=pic, kf=kf, dev=dev, **sw)
    _check(w, h, fmt, quality, frames, hdr, got, cuts, pic=pic, kf=kf, modes=sw.get("modes", False), bqi=sw.get("bqi", 0))
    if kf == 4:   # the interval restarts at the cut: frame 7 is a key frame by the interval, and not measured; frame 4 is not
        assert [g["inter"]["key"] for g in got] == [1, 0, 0, 1, 0, 0, 0, 1, 0]
        assert [g["cut"]["measured"] for g in got] == [0, 1, 1, 1, 1, 1, 1, 0, 1]
    if sw.get("pack"):
        assert all(g["pack"]["device"] == 1 for g in got)


@pytest.mark.gpu
def test_duplicates_before_the_cut(hip):
    """Two duplicates asked for the frame before the cut: their granules count on, the cut frame's starts a new key frame."""
    w, h, fmt, q = 176, 144, 0, 32
    frames = CR.scene(w, h, fmt, 5, 3)
    hdr, got = _encode(w, h, fmt, q, frames, dups={2: 2})
    _check(w, h, fmt, q, frames, hdr, got, [3], dups={2: 2})
    assert [g["gp"] for g in got] == [64, 65, 66, 67, 68, 6 << 6, (6 << 6) + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("modes", [False, True], ids=["five_modes", "eight_modes"])
def test_bitrate_mode_equals_the_restatement(hip, modes):
    """The decision ahead of the probe, the probe (key or inter accordingly) on the measurement's statistics, the controller's record,
    the packets and the cut statistics."""
    w, h, fmt, bitrate = 176, 144, 0, 400000
    frames = CR.scene(w, h, fmt, 5, 2)
    hdr, got = _encode(w, h, fmt, 32, frames, modes=modes, bitrate=bitrate)
    rs = CR.CutRateStream(T, w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, kf_interval=64, modes=modes)
    want = []
    try:
        for fr in frames:
            want.extend(rs.frame(fr))
    finally:
        rs.close()
    assert len(got) == len(want)
    for k, (g, (wpkt, rec, cst)) in enumerate(zip(got, want)):
        for name, v in rec.items():
            assert g["rate"][name] == v, (k, name, g["rate"][name], v)
        assert {n: g["cut"][n] for n in CUT_FIELDS} == {n: cst[n] for n in CUT_FIELDS}, (k, g["cut"], cst)
        assert g["pkt"] == wpkt, k
    assert [g["rate"]["key"] for g in got] == [1, 0, 1, 0, 0] and [g["cut"]["cut"] for g in got] == [0, 0, 1, 0, 0]
    assert [g["gp"] for g in got] == [64, 65, 3 << 6, (3 << 6) + 1, (3 << 6) + 2]


@functools.lru_cache(maxsize=None)
def _never_cuts(kind, w, h, bitrate, t):
    hdr, got = _encode(w, h, 0, 32, CR.clip(kind, w, h, 0, 5, seed=3), t=t, bitrate=bitrate)
    return hdr, got


@pytest.mark.gpu
@pytest.mark.parametrize("bitrate", [None, 300000], ids=["quality", "bitrate"])
@pytest.mark.parametrize("kind,w,h", [("pan", 176, 144), ("static", 176, 144), ("pan", 352, 288)])
def test_no_cut_gives_the_packets_of_the_switch_off(hip, kind, w, h, bitrate):
    """Every inter frame is measured and none cuts: the frames are coded from the measurement's statistics (k_enc_mb_modes; in bitrate
    mode the probe too), and every packet, statistic and reconstruction is the one the encoder makes with the switch off."""
    (hdr_on, on), (hdr_off, off) = _never_cuts(kind, w, h, bitrate, T), _never_cuts(kind, w, h, bitrate, 0)
    assert hdr_on == hdr_off and len(on) == len(off) == 5
    assert [g["cut"]["measured"] for g in on] == [0, 1, 1, 1, 1] and not any(g["cut"]["cut"] for g in on)
    assert not any(g["cut"]["measured"] or g["cut"]["ratio"] or g["cut"]["measure_ms"] for g in off)
    for f, (a, b) in enumerate(zip(on, off)):
        assert a["pkt"] == b["pkt"] and a["gp"] == b["gp"] and a["inter"] == b["inter"], f
        for p in range(3):
            assert np.array_equal(a["recon"][p], b["recon"][p]), (f, p)
        if bitrate:
            assert {k: v for k, v in a["rate"].items() if k not in RATE_TIMES} == {k: v for k, v in b["rate"].items() if k not in RATE_TIMES}, f
    assert any(g["inter"]["modes"]["INTER_MV"] for g in on) or kind == "static"


@functools.lru_cache(maxsize=None)
def _scene_stream(dev=False):
    w, h, fmt = 176, 144, 0
    return _encode(w, h, fmt, 32, CR.scene(w, h, fmt, 6, 3), dev=dev)


@pytest.mark.gpu
def test_a_decoder_can_start_at_the_cut(hip):
    """Seeking: a fresh decoder fed the headers and then the packets from the cut key frame on shows the pictures of a decoder that
    saw the whole stream."""
    from theora_amd.decoder import Decoder
    hdr, got = _scene_stream()
    assert [g["inter"]["key"] for g in got] == [1, 0, 0, 1, 0, 0]
    whole, late = Decoder(hdr), Decoder(hdr)
    try:
        for f, g in enumerate(got):
            rc, gp = whole.packetin(g["pkt"])
            assert gp == g["gp"]
            pic = whole.ycbcr_out()
            if f < 3:
                continue
            assert late.packetin(g["pkt"])[0] == rc   # (its granules count from where it started)
            seen = late.ycbcr_out()
            for p in range(3):
                assert np.array_equal(seen[p], pic[p]) and np.array_equal(seen[p], g["recon"][p]), (f, p)
    finally:
        whole.close()
        late.close()


@pytest.mark.gpu
def test_cut_stream_decodes_in_the_reference(hip):
    """The GPU encoder's `scene` stream through the reference decoder: no packet refused, its granules (the cut's a key frame's) and
    its pictures are the encoder's."""
    from oracle import ref
    from tests import refcmp
    refcmp.need_ref()
    hdr, got = _scene_stream()
    rd = ref.RefDecoder(hdr)
    try:
        for f, g in enumerate(got):
            rc, gp = rd.packetin(g["pkt"])
            assert rc == 0 and gp == g["gp"], (f, rc, gp)
            assert (gp & 63 == 0) == (f in (0, 3))
            assert not refcmp.diff_planes(rd.ycbcr_out(), g["recon"]), f
            refcmp.TALLY["frames"] += 1
    finally:
        rd.close()


@pytest.mark.gpu
def test_host_and_device_input_give_the_same_packets(hip):
    (_, host), (_, dev) = _scene_stream(), _scene_stream(dev=True)
    assert [g["pkt"] for g in host] == [g["pkt"] for g in dev]
    for a, b in zip(host, dev):
        assert {n: a["cut"][n] for n in CUT_FIELDS} == {n: b["cut"][n] for n in CUT_FIELDS}


@pytest.mark.gpu
def test_switch_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, Encoder
    e = Encoder(64, 48, 0, 30, inter=True)
    e.header_packets()
    assert e.ctl(TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, T)[0] == 0
    e.encode(CR.scene(64, 48, 0, 1, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, T)[0] == -10
    assert e.cut_stats()["ratio"] == T
    e.close()
