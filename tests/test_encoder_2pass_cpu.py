"""th_encode_* two-pass without a GPU (include/theoraenc_hip.h, "Two-pass"): the calling conventions and refusals of
TH_ENCCTL_THIP_2PASS_OUT / _IN / _GET_2PASS_STATS, none of which touches a device (on a machine without one, a call that tried
would answer TH_EFAULT, not the code asserted); the pass file's codec; the count _2PASS_IN(NULL) answers; and the second pass's
controller on planted curves, against tests/enc_rate_ref.py's one-pass controller."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import enc_2pass_ref as TP

ENOTFORMAT = -21
W, H = 64, 48


def _enc(**kw):
    from theora_amd import _lib as Lm
    from theora_amd.encoder import Encoder
    return Lm, Encoder(W, H, 0, 32, **kw)


def _fields(inter=False, fps=(30, 1), shift=6):
    return TP.fields_of(W, H, (0, 0, W, H), 0, fps, shift, inter)


def _out(e, size=None, null=False):
    from theora_amd import encoder as E
    p = C.POINTER(C.c_ubyte)()
    rc = e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_2PASS_OUT, None if null else C.byref(p), C.sizeof(p) if size is None else size)
    return rc, (C.string_at(p, rc) if rc > 0 else b"")


def _in(e, data):
    from theora_amd import encoder as E
    if data is None:
        return e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_2PASS_IN, None, 0)
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data or b"\0")
    return e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_2PASS_IN, buf, len(data))


def _submit(e):
    """th_encode_ycbcr_in, TH_ENCCTL_THIP_YCBCR_IN_DEVICE and TH_ENCCTL_THIP_RGB_IN with well-formed arguments -> their codes."""
    from theora_amd import encoder as E
    from theora_amd._lib import ThImgPlane
    planes = [np.zeros((H, W), np.uint8), np.zeros((H // 2, W // 2), np.uint8), np.zeros((H // 2, W // 2), np.uint8)]
    buf = (ThImgPlane * 3)()
    dev = E.DeviceIn()
    for p, a in enumerate(planes):
        for b in (buf[p], dev.planes[p]):
            b.width, b.height, b.stride = a.shape[1], a.shape[0], a.strides[0]
            b.data = a.ctypes.data_as(C.POINTER(C.c_ubyte))
    rgb = np.zeros((H, W, 3), np.uint8)
    r = E.RgbIn()
    r.format, r.device, r.width, r.height = E.RGB_FORMATS["rgb"], 0, W, H
    r.src[0], r.pitch[0] = rgb.ctypes.data, rgb.strides[0]
    return (e._L.th_encode_ycbcr_in(e._enc, buf),
            e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_YCBCR_IN_DEVICE, C.byref(dev), C.sizeof(dev)),
            e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_RGB_IN, C.byref(r), C.sizeof(r)))


# ---- the calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(bitrate=100000), dict(inter=True, keyframe_interval=12)], ids=["quality", "bitrate", "inter"])
def test_2pass_out_enters_pass_one_in_either_mode(kw):
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_2PASS_OUT, E.TH_ENCCTL_THIP_2PASS_IN, E.TH_ENCCTL_THIP_GET_2PASS_STATS) == (0x721D, 0x721B, 0x721C)
    Lm, e = _enc(**kw)
    try:
        p = C.POINTER(C.c_ubyte)()
        assert e._L.th_encode_ctl(e._enc, 0x721A, C.byref(p), C.sizeof(p)) == Lm.EIMPL   # not used: an unknown request
        assert e.two_pass_stats()["pass"] == 0
        for size in (0, 4, 7, 16):
            assert _out(e, size=size)[0] == Lm.EINVAL, size
        assert _out(e, null=True)[0] == Lm.EFAULT
        assert e.two_pass_stats()["pass"] == 0
        rc, data = _out(e)
        assert rc == TP.HEADER_BYTES and data == TP.pack_header(_fields(inter=bool(kw.get("inter"))))
        assert e.two_pass_stats()["pass"] == 1
        assert _out(e) == (0, b"")                 # no packet yet: nothing to say
        assert e.two_pass_out() == b""
        assert _in(e, data) == Lm.EINVAL           # both on one context
        assert _in(e, None) == Lm.EINVAL
    finally:
        e.close()


def test_2pass_in_refusals():
    from theora_amd import encoder as E
    Lm, e = _enc()
    try:
        good = TP.pack_header(_fields())
        assert _in(e, good) == Lm.EINVAL and _in(e, None) == Lm.EINVAL      # quality mode
        assert e.two_pass_stats()["pass"] == 0
        e.set_bitrate(100000)
        for bad in (b"THP1" + good[4:], b"OggS" + good[4:], good[:4] + struct.pack("<I", 2) + good[8:], b"\0" * 8):
            assert _in(e, bad) == ENOTFORMAT
            assert e.two_pass_stats()["pass"] == 0 and _in(e, None) == TP.HEADER_BYTES
            assert _in(e, b"") == 0
        assert _in(e, b"THP") == 3 and _in(e, b"X" + good[4:]) == ENOTFORMAT   # across chunks; and the context starts over
        for k in range(11):   # geometry, fps, shift, the inter-frame switch: each field alone
            f = _fields()
            f[k] += 1
            assert _in(e, TP.pack_header(f, 3, 0)) == Lm.EINVAL, k
        assert _in(e, good) == TP.HEADER_BYTES     # 0 frames: nothing more is taken, and no frame may come
        assert _in(e, b"\0" * 10) == 0 and _in(e, None) == 0
        assert _submit(e) == (Lm.EINVAL,) * 3
        assert _out(e)[0] == Lm.EINVAL             # both on one context
        st = e.two_pass_stats()
        assert st["pass"] == 2 and st["frame"] == 0 and st["fresh"] == [0] * 64
        s = E.TwoPassStats()
        assert e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_GET_2PASS_STATS, C.byref(s), C.sizeof(s) - 8) == Lm.EINVAL
        assert e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_GET_2PASS_STATS, None, C.sizeof(s)) == Lm.EINVAL
        for req in (24, 26):                        # libtheora's numbers stay TH_EIMPL
            assert e.ctl(req, 0)[0] == Lm.EIMPL
        for req, v in ((E.TH_ENCCTL_SET_RATE_FLAGS, 0), (E.TH_ENCCTL_SET_RATE_BUFFER, 20)):   # accepted in pass 2
            assert e.ctl(req, v)[0] == 0
    finally:
        e.close()


def test_inter_switch_must_match():
    Lm, e = _enc(bitrate=100000, inter=True, keyframe_interval=12)
    try:
        assert _in(e, TP.pack_header(_fields(inter=False), 2, 0)) == Lm.EINVAL
        assert _in(e, TP.pack_header(_fields(inter=True), 2, 0)) == TP.HEADER_BYTES
    finally:
        e.close()


def test_frames_wait_for_their_records():
    """No frame is taken while its record has not arrived; the refusal comes before the device (there is none here)."""
    Lm, e = _enc(bitrate=100000)
    try:
        recs = [TP.pack_record(TP.KEY, 30, 8000, [1000 * (q + 1) for q in range(64)]) for _ in range(2)]
        data = TP.finish_header(_fields(), [TP.unpack_record(r) for r in recs]) + b"".join(recs)
        assert _in(e, None) == TP.HEADER_BYTES
        assert _submit(e) == (Lm.EINVAL,) * 3
        assert _in(e, data[:TP.HEADER_BYTES]) == TP.HEADER_BYTES
        assert _submit(e) == (Lm.EINVAL,) * 3
        assert _in(e, data[TP.HEADER_BYTES:-1]) == 2 * TP.RECORD_BYTES - 1     # ahead of time, and the first record is whole:
        assert _in(e, None) == 0                                               # the gate is open (a device would be next)
        assert _in(e, data[-1:] + b"more") == 1                                # nothing beyond the header's count is taken
    finally:
        e.close()


@pytest.mark.parametrize("chunk", [1, 7, TP.RECORD_BYTES, 10 ** 6])
def test_2pass_in_null_counts_down(chunk):
    Lm, e = _enc(bitrate=100000)
    try:
        recs = [TP.unpack_record(TP.pack_record(k % 2, 20 + k, 999 * k, [k * q for q in range(64)])) for k in range(3)]
        data = TP.finish_header(_fields(), recs) + b"".join(TP.pack_record(r["type"], r["qi"], r["bits"], r["E"]) for r in recs)
        hdr, have = None, 0
        assert _in(e, None) == TP.wanted(0, None, 0) == TP.HEADER_BYTES
        while have < len(data):
            part = data[have:have + chunk]
            assert _in(e, part) == len(part)
            have += len(part)
            if have >= TP.HEADER_BYTES:
                hdr = TP.unpack_header(data[:TP.HEADER_BYTES])
            assert _in(e, None) == TP.wanted(have, hdr, 0), have
        assert _in(e, None) == 0 and have == TP.HEADER_BYTES + 3 * TP.RECORD_BYTES
    finally:
        e.close()


# ---- the codec ------------------------------------------------------------------------------------------------------------------
def test_record_codec_round_trips_and_saturates():
    rng = np.random.default_rng(3)
    for rtype in (TP.KEY, TP.INTER, TP.DUP, TP.DROPPED):
        E = [int(x) for x in rng.integers(0, 1 << 32, 64)]
        r = TP.unpack_record(TP.pack_record(rtype, 17, 123456, E))
        assert r == dict(type=rtype, qi=17, bits=123456, E=E)
    r = TP.unpack_record(TP.pack_record(TP.KEY, 63, 1 << 40, [(1 << 32) - 1, 1 << 32, 1 << 50, -5] + [0] * 60))
    assert r["bits"] == TP.U32 and r["E"][:4] == [TP.U32, TP.U32, TP.U32, 0]
    assert len(TP.pack_record(0, 0, 0, [0] * 64)) == TP.RECORD_BYTES
    with pytest.raises(TP.Truncated):
        TP.unpack_record(b"\0" * (TP.RECORD_BYTES - 1))


def test_header_codec_round_trips_and_rejects():
    recs = [dict(type=t, qi=9, bits=80, E=[(k + 1) * (q + 1) * 10 ** 7 for q in range(64)]) for k, t in
            enumerate((TP.KEY, TP.INTER, TP.DUP, TP.INTER, TP.DROPPED, TP.KEY))]
    for inter in (False, True):
        f = _fields(inter=inter)
        h = TP.unpack_header(TP.finish_header(f, recs))
        assert h["fields"] == f and h["frames"] == 5 and h["dups"] == 1
        want = [[0] * 64, [0] * 64]
        for r in recs:
            c = TP.rec_class(r["type"], inter)
            if c is not None:
                want[c] = [a + b for a, b in zip(want[c], r["E"])]
        assert h["tot"] == want and max(want[0]) > 1 << 32       # the sums are 64 bits wide
    data = TP.finish_header(_fields(), recs)
    assert len(data) == TP.HEADER_BYTES == len(TP.pack_header(_fields()))
    with pytest.raises(TP.NotFormat):
        TP.unpack_header(b"THQ2" + data[4:])
    with pytest.raises(TP.NotFormat):
        TP.unpack_header(data[:4] + struct.pack("<I", 0) + data[8:])
    with pytest.raises(TP.Truncated):
        TP.unpack_header(data[:-1])
    body = b"".join(TP.pack_record(r["type"], r["qi"], r["bits"], r["E"]) for r in recs)
    assert TP.parse(data + body)[1] == recs
    for cut in (data + body[:-1], data + body[:-TP.RECORD_BYTES], data + body + body[:TP.RECORD_BYTES]):
        with pytest.raises(TP.Truncated):
            TP.parse(cut)


# ---- the controller on planted curves --------------------------------------------------------------------------------------------------
def _planted(curves, T, scale=1, rule="scale"):
    """Pass 2 over frames (all key frames, inter frames off) whose records and fresh probes are `curves`, each packet taking
    scale x Rec[qi] bits -> (qis, total bits, B, controller)."""
    recs = [dict(type=TP.KEY, qi=0, bits=0, E=list(E)) for E in curves]
    hdr = TP.unpack_header(TP.finish_header(_fields(fps=(1, 1)), recs))
    ctl = TP.Controller2(T, (1, 1), hdr, rule)
    qis, total = [], 0
    for r in recs:
        qi = ctl.choose(r, r["E"], True)
        A = scale * r["E"][qi]
        ctl.coded(True, qi, A)
        qis.append(qi)
        total += A
    return qis, total, ctl.B, ctl


def test_equal_curves_one_qi_and_the_budget_met():
    """A_n = Rec_n[qi] and equal curves with a step of 1000 bits between adjacent qi: B = N E[40] + 200 holds N frames at qi 40 and
    no frame at 41, so every frame gets 40 and the total is under B by 200, less than one frame's step."""
    E = [1000 * (q + 1) for q in range(64)]
    N = 20
    qis, total, B, ctl = _planted([E] * N, E[40] + 10)
    assert B == N * E[40] + 200
    assert qis == [40] * N
    assert 0 <= B - total < 1000
    assert ctl.c == [65536, 65536] and ctl.ratio == [65536, 65536]


def test_alternating_curves_keep_one_qi_where_one_pass_moves():
    easy, hard = [500 * (q + 1) for q in range(64)], [3000 * (q + 1) for q in range(64)]
    curves = [easy, hard] * 12
    N = len(curves)
    B = 12 * (easy[30] + hard[30]) + 240        # holds the file at qi 30 with less than the last frame's step to spare
    assert B % N == 0
    qis, total, B2, _ = _planted(curves, B // N)
    assert B2 == B and qis == [30] * N and 0 <= B - total < 500
    one = TP.OnePass(B // N, (1, 1), False, 1, 6)
    oq = []
    for f, E in enumerate(curves):
        qi = one.choose(E, True, f, f)
        one.coded(True, qi, E[qi])
        oq.append(qi)
    print("one-pass qi on the same curves:", oq)
    assert max(oq) - min(oq) > 0


def test_doubled_packets_converge():
    """A_n = 2 Rec_n[qi] throughout (the fresh curves equal to the recorded ones): the correction c_key converges on 2.0, the
    fresh-to-recorded ratio stays 1.0, and the total stays within the one-pass bound R / 2 + T (R = 12 T, the default buffer) of B.
    The rule first proposed (Controller2's rule="halving": its r_0 converges on 2.0) meets the same bound."""
    E = [1000 + 200 * q for q in range(64)]
    N = 24
    T = 2 * E[32]
    qis, total, B, ctl = _planted([E] * N, T, scale=2)
    print("qi", qis, "total - B", total - B, "c", ctl.c)
    assert abs(ctl.c[0] - 131072) <= 131072 // 100 and ctl.c[1] == 65536 and ctl.ratio == [65536, 65536]
    assert abs(total - B) <= 12 * T // 2 + T
    qis, total, B, ctl = _planted([E] * N, T, scale=2, rule="halving")
    assert abs(ctl.r[0] - 131072) <= 131072 // 100 and ctl.r[1] == 65536
    assert abs(total - B) <= 12 * T // 2 + T
