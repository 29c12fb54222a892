"""th_encode_*'s automatic key frames without a GPU: the two controls (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES,
TH_ENCCTL_THIP_GET_CUT_STATS), the statistics' layout, the Python face, and the rule itself on tests/enc_cut_ref.py's restatement:
which frames of the test clips it makes key frames, that the reference decoder takes such a stream and calls the cut packet a key
frame, and that a key frame at a cut never costs bytes on these clips.  Nothing here reaches the first th_encode_ycbcr_in, so nothing
touches the GPU (this machine may have none); that a call after the first frame is refused is tests/test_gpu_encoder_cut.py's to show."""
import ctypes as C
import functools
import os
import re

import pytest

from tests import enc_cut_ref as CR
from tests import enc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH_EINVAL, TH_EIMPL = -10, -23
W, H, FMT, T = 176, 144, 0, CR.RECOMMENDED


def _enc():
    from theora_amd import _lib
    from theora_amd.encoder import make_info
    L = _lib.load()
    info = make_info(64, 48, 0, 32)
    enc = L.th_encode_alloc(C.byref(info))
    assert enc
    return L, enc


def _ctl(L, enc, req, value, ctype=C.c_int):
    v = ctype(value)
    return L.th_encode_ctl(enc, req, C.byref(v), C.sizeof(v)), v.value


def test_constants_and_layout_agree_with_the_header():
    from theora_amd import encoder as E
    hdr = open(os.path.join(ROOT, "include", "theoraenc_hip.h")).read()
    assert (E.TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, E.TH_ENCCTL_THIP_GET_CUT_STATS) == (0x720F, 0x7210)
    for name in ("TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES", "TH_ENCCTL_THIP_GET_CUT_STATS"):
        m = re.search(r"#define %s \((0x[0-9A-Fa-f]+)\)" % name, hdr)
        assert m and int(m.group(1), 16) == getattr(E, name), name
    body = re.search(r"typedef struct thip_enc_cut_stats \{(.*?)\} thip_enc_cut_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(int32_t|int64_t|double)\s+(\w+);", body)]
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(E.CutStats._fields_)
    assert C.sizeof(E.CutStats) == 40
    assert "Automatic key frames" in hdr and E.AUTO_KEYFRAMES_DEFAULT == CR.RECOMMENDED == 230


def test_auto_keyframe_controls():
    """0, 1, 230 and 4096 accepted, -1 and 4097 TH_EINVAL; accepted with inter frames off and on; GET_CUT_STATS answers before any
    frame: all zero but the ratio in force; 0x7299 is still unknown."""
    from theora_amd import encoder as E
    L, enc = _enc()
    try:
        s = E.CutStats()
        C.memset(C.byref(s), 0xFF, C.sizeof(s))
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_CUT_STATS, C.byref(s), C.sizeof(s)) == 0
        assert bytes(s) == bytes(C.sizeof(s))
        for v in (1, 230, 4096, 0, 230):   # (inter frames are off here)
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, v) == (0, v)
        for v in (-1, 4097, 1 << 20, -(1 << 31)):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, v)[0] == TH_EINVAL, v
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, 1, C.c_int64)[0] == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_CUT_STATS, C.byref(s), C.sizeof(s)) == 0
        assert (s.measured, s.cut, s.intra_mbs, s.ratio, s.pred, s.intra, s.measure_ms) == (0, 0, 0, 230, 0, 0, 0.0)
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_CUT_STATS, C.byref(s), C.sizeof(s) - 4) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_CUT_STATS, None, C.sizeof(s)) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES, 4096) == (0, 4096)
        assert _ctl(L, enc, 0x7299, 0)[0] == TH_EIMPL   # (still pinned)
    finally:
        L.th_encode_free(enc)


def test_headers_do_not_change_and_the_python_face():
    from theora_amd.encoder import AUTO_KEYFRAMES_DEFAULT, Encoder
    want = None
    for inter in (False, True):
        for ak, t in ((None, 0), (False, 0), (True, AUTO_KEYFRAMES_DEFAULT), (1, 1), (4096, 4096)):
            e = Encoder(W, H, FMT, 32, inter=inter, auto_keyframes=ak)
            hdr = e.header_packets()
            st = e.cut_stats()
            e.close()
            assert e.auto_keyframes == t
            assert st == dict(measured=0, cut=0, intra_mbs=0, ratio=t, pred=0, intra=0, measure_ms=0.0)
            want = want or hdr
            assert hdr == want, (inter, ak)
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            Encoder(W, H, FMT, 32, inter=True, auto_keyframes=bad)


def test_decide():
    """256 P >= t I and P >= 4 * 256 nmbs, both inclusive; t = 0 never."""
    n = 99
    assert CR.decide(230 * 1000, 256 * 1000, n, 230) and not CR.decide(230 * 1000 - 1, 256 * 1000, n, 230)
    assert CR.decide(1024 * n, 1, n, 230) and not CR.decide(1024 * n - 1, 1, n, 230)
    assert CR.decide(1 << 40, 1 << 40, n, 256) and not CR.decide(1 << 40, (1 << 40) + 1, n, 256)
    assert not CR.decide(1 << 40, 1, n, 0)


# ---- the restatement on the test clips: one stream a (clip, quality, ratio), shared by the tests below ------------------------------------
NFRAMES = {"scene": 8, "cut": 6, "pan": 6, "static": 4, "flat_noise": 4}


@functools.lru_cache(maxsize=None)
def _setup():
    from theora_amd.encoder import Encoder
    e = Encoder(W, H, FMT, 32)
    hdr = e.header_packets()
    e.close()
    return hdr, enc_ref.SetupParams(hdr[2])


@functools.lru_cache(maxsize=None)
def _stream(kind, q, t):
    """Per frame (packet, key, cut statistics, reconstruction) of the restated five-mode encoder, interval 64."""
    enc = CR.encoder(t, W, H, FMT, (0, 0, W, H), _setup()[1], 64, 6)
    out = []
    try:
        for fr in CR.clip(kind, W, H, FMT, NFRAMES[kind], seed=0, cut=3):
            r = enc.frame(fr, q)
            out.append((r["packet"], r["key"], r["cut"], enc.recon))
    finally:
        enc.close()
    return out


@pytest.mark.parametrize("q", [16, 48])
@pytest.mark.parametrize("kind,cuts", [("pan", []), ("static", []), ("flat_noise", []), ("scene", [3]), ("cut", [3, 4, 5])])
def test_decisions_on_the_test_clips(kind, cuts, q):
    out = _stream(kind, q, T)
    for f, (pkt, key, st, _) in enumerate(out):
        print(kind, q, f, st, "P/I %.3f" % (st["pred"] / max(st["intra"], 1)), "P/(256 nmbs) %.2f" % (st["pred"] / (256 * 99)))
    assert [f for f, o in enumerate(out) if o[2]["cut"]] == cuts
    assert [f for f, o in enumerate(out) if o[1]] == [0] + cuts
    # every frame but the first is an inter frame by the interval rule, so it is measured
    assert [o[2]["measured"] for o in out] == [0] + [1] * (len(out) - 1)
    assert all(o[2]["ratio"] == T for o in out)


@pytest.mark.parametrize("q", [16, 32, 48])
@pytest.mark.parametrize("kind", ["scene", "cut"])
def test_a_cut_key_frame_costs_no_bytes(kind, q):
    on, off = _stream(kind, q, T), _stream(kind, q, 0)
    assert [o[1] for o in off] == [True] + [False] * (len(off) - 1) and not any(o[2]["measured"] for o in off)
    b_on, b_off = sum(len(o[0]) for o in on), sum(len(o[0]) for o in off)
    print(kind, q, "inter frames only %d bytes, key frames at the cuts %d" % (b_off, b_on))
    assert b_on <= b_off
    if kind == "scene":   # only the cut frame's packet differs: all its macro blocks are INTRA either way, so the reconstruction is one
        assert [o[0] for f, o in enumerate(on) if f != 3] == [o[0] for f, o in enumerate(off) if f != 3]


def test_the_reference_decoder_takes_the_cut_stream():
    """The reference decoder accepts the restated `scene` stream, reports a key frame's granule for the cut packet and shows the
    restatement's reconstruction after every packet."""
    from oracle import ref
    from tests import refcmp
    refcmp.need_ref()
    out = _stream("scene", 32, T)
    assert [o[1] for o in out] == [True, False, False, True, False, False, False, False]
    rd = ref.RefDecoder(_setup()[0])
    try:
        for f, (pkt, key, st, recon) in enumerate(out):
            rc, gp = rd.packetin(pkt)
            assert rc == 0, (f, rc)
            assert (gp & 63 == 0) == key and gp >> 6 == (4 if f >= 3 else 1), (f, gp)
            assert (pkt[0] & 0x40 == 0) == key
            assert not refcmp.diff_planes(rd.ycbcr_out(), recon), f
            refcmp.TALLY["frames"] += 1
    finally:
        rd.close()
