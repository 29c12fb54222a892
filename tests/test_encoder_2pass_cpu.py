"""th_encode_* two-pass without a GPU (include/theoraenc_hip.h, "Two-pass"): the calling conventions and refusals of
TH_ENCCTL_THIP_2PASS_OUT / _IN / _GET_2PASS_STATS, none of which touches a device (on a machine without one, a call that tried
would answer TH_EFAULT, not the code asserted); the pass file's codec; the count _2PASS_IN(NULL) answers; and the second pass's
controller on planted curves, against tests/enc_rate_ref.py's one-pass controller.  Then the library's own pass-file writer, reader
and second controller (theora_amd/csrc/thip_ratectl.h's TwoPass), replayed by tests/native/ratectl_host.cpp under AddressSanitizer
and UBSan and compared byte by byte and field by field with the restatement (tests/ratectl_host.py)."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import enc_2pass_ref as TP
from tests import ratectl_host as RH

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


# ---- the library's TwoPass, replayed on the host (tests/ratectl_host.py) ------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return RH.build(tmp_path_factory)


def _frames(got):
    return [d for step, d in got if step == "frame"]


def _file(fields, recs):
    return TP.finish_header(fields, recs) + b"".join(TP.pack_record(r["type"], r["qi"], r["bits"], r["E"]) for r in recs)


@pytest.mark.parametrize("inter", [False, True], ids=["intra", "inter"])
@pytest.mark.parametrize("mode", ["quality", "bitrate"])
def test_pass_one_writes_the_restatements_bytes(host, tmp_path, mode, inter):
    """The placeholder, every packet's record and the finished header are pack_header's, pack_record's and finish_header's bytes
    (Model.run compares them), and between them TH_ENCCTL_THIP_2PASS_OUT has nothing to say.  Quality mode: probe entries above
    2^32 - 1 and below 0 (the record saturates and clamps them) and a packet whose bits saturate the record's u32.  Bitrate mode:
    the controller's drops are records of type 3."""
    m = RH.Model(inter=inter, K=4 if inter else 1, quality=17)
    easy = [500 * (q + 1) for q in range(64)]
    wild = [(1 << 32) + 5, 1 << 50, -7, (1 << 32) - 1] + easy[4:]
    if mode == "bitrate":
        m.bitrate(30 * 10000)
    assert m.out() == TP.pack_header(m.fields) and m.out() == b""
    for f in range(12):
        dups = 2 if f == 2 else 1 if f == 7 else 0
        if mode == "bitrate":
            m.frame(easy, dups=dups, mul=0, add=80000)
        else:
            m.frame(wild if f % 2 else easy, dups=dups, mul=0, add=1 << 35 if f == 5 else 8000 * (f + 1))
        assert len(m.out()) == TP.RECORD_BYTES
        for _ in range(dups):
            m.dup()
            assert len(m.out()) == TP.RECORD_BYTES
        assert m.out() == b""
    m.done()
    final = m.out()
    assert m.out() == b""
    m.run(host, tmp_path)
    h, recs = TP.parse(_file(m.fields, m.records))
    assert final == TP.finish_header(m.fields, recs) and h["dups"] == 3 and h["frames"] == 12
    want = {TP.KEY, TP.DUP} | ({TP.INTER} if inter else set()) | ({TP.DROPPED} if mode == "bitrate" else set())
    assert {r["type"] for r in recs} == want
    if mode == "quality":
        assert recs[1]["E"][:4] == [TP.U32, TP.U32, 0, TP.U32] and TP.U32 in [r["bits"] for r in recs]
        assert max(h["tot"][1 if inter else 0]) > 1 << 32


PASS2_RECS = [dict(type=t, qi=20 + k, bits=999 * k, E=[0] * 64 if t == TP.DUP else [(k + 1) * (q + 1) for q in range(64)])
              for k, t in enumerate((TP.KEY, TP.DUP, TP.KEY, TP.KEY))]


@pytest.mark.parametrize("chunk", [1, 7, TP.RECORD_BYTES, 10 ** 6])
def test_pass_two_takes_the_file_in_chunks(host, tmp_path, chunk):
    """After every chunk the bytes consumed and the count TH_ENCCTL_THIP_2PASS_IN(NULL) answers are the restatement's; a frame is
    refused exactly while its record is missing, and after the file's last."""
    m = RH.Model()
    m.bitrate(100000)
    data = _file(m.fields, PASS2_RECS)
    frames = [(PASS2_RECS[0]["E"], 1), (PASS2_RECS[2]["E"], 0), (PASS2_RECS[3]["E"], 0)]
    assert m.wanted() == TP.HEADER_BYTES and m.gate() == RH.EINVAL
    have = 0
    while have < len(data):
        part = data[have:have + chunk]
        assert m.feed(part) == len(part)
        have += len(part)
        m.wanted()
        while frames:
            n = m._n()
            assert (m.gate() == 0) == (have >= TP.HEADER_BYTES + (n + 1) * TP.RECORD_BYTES), (have, n)
            if m.gate():
                break
            E, dups = frames.pop(0)
            assert m.frame(E, dups=dups) is not None
            m.wanted()
            for _ in range(dups):
                m.dup()
    assert not frames and m.gate() == RH.EINVAL and m.frame(PASS2_RECS[0]["E"]) is None   # after the last
    assert m.feed(b"more") == 0 and m.wanted() == 0
    m.run(host, tmp_path)


def test_pass_two_refuses_a_bad_header_and_starts_over(host, tmp_path):
    """A bad magic or version: TH_ENOTFORMAT as soon as 8 bytes are in; each of the eleven fields mismatched: TH_EINVAL.  After
    either the object is as before the first byte (Model.run compares its state), and a good file is then accepted."""
    m = RH.Model()
    m.bitrate(100000)
    good = _file(m.fields, PASS2_RECS)
    for bad in (b"THP1" + good[4:], good[:4] + struct.pack("<I", 2) + good[8:]):
        assert m.feed(bad[:7]) == 7 and m.feed(bad[7:20]) == RH.ENOTFORMAT
        assert m.feed(bad) == RH.ENOTFORMAT and m.wanted() == TP.HEADER_BYTES
    for k in range(11):
        f = list(m.fields)
        f[k] += 1
        assert m.feed(TP.pack_header(f, 3, 1)[:-1]) == TP.HEADER_BYTES - 1 and m.feed(b"\0" + good[TP.HEADER_BYTES:]) == RH.EINVAL, k
    assert m.feed(good) == len(good) and m.gate() == 0
    assert m.frame(PASS2_RECS[0]["E"], dups=1) is not None
    m.run(host, tmp_path)


def _replayed(host, tmp_path, recs, fresh, T, scale=1, **kw):
    """Pass 2 over `recs` with the fresh probes `fresh` (one a record), each packet taking scale x E[qi] bits: the library's
    controller against Controller2 (Model.run compares qi, estimate, budget left, recorded_left, the ratios and the corrections
    of every frame) -> the model and the frames' lines."""
    m = RH.Model(fps=(1, 1), **kw)
    m.bitrate(T)
    data = _file(m.fields, recs)
    assert m.feed(data) == len(data)
    for k, r in enumerate(recs):
        if r["type"] == TP.DUP:
            m.dup()
        else:
            dups = 0
            while k + dups + 1 < len(recs) and recs[k + dups + 1]["type"] == TP.DUP:
                dups += 1
            assert m.frame(fresh[k], dups=dups, mul=scale) is not None
    return m, _frames(m.run(host, tmp_path))


def _key_recs(curves):
    return [dict(type=TP.KEY, qi=0, bits=0, E=list(E)) for E in curves]


def test_library_on_equal_curves(host, tmp_path):
    E = [1000 * (q + 1) for q in range(64)]
    m, fr = _replayed(host, tmp_path, _key_recs([E] * 20), [E] * 20, E[40] + 10)
    assert [d["qi"] for d in fr] == _planted([E] * 20, E[40] + 10)[0] == [40] * 20
    assert fr[-1]["c"] == [65536, 65536] and fr[-1]["tp_corr"] == [65536] * 4 and 0 <= fr[-1]["budget_left"] < 1000


def test_library_on_alternating_curves(host, tmp_path):
    easy, hard = [500 * (q + 1) for q in range(64)], [3000 * (q + 1) for q in range(64)]
    curves = [easy, hard] * 12
    T = (12 * (easy[30] + hard[30]) + 240) // 24
    m, fr = _replayed(host, tmp_path, _key_recs(curves), curves, T)
    assert [d["qi"] for d in fr] == _planted(curves, T)[0] == [30] * 24 and 0 <= fr[-1]["budget_left"] < 500


def test_library_on_doubled_packets(host, tmp_path):
    E = [1000 + 200 * q for q in range(64)]
    m, fr = _replayed(host, tmp_path, _key_recs([E] * 24), [E] * 24, 2 * E[32], scale=2)
    qis, total, B, ctl = _planted([E] * 24, 2 * E[32], scale=2)
    assert [d["qi"] for d in fr] == qis and fr[-1]["budget_left"] == B - total
    assert fr[-1]["tp_corr"] == ctl.c + [65536, 65536] and abs(fr[-1]["c"][0] - 131072) <= 131072 // 100


def test_library_on_mixed_records_and_fresh_curves_half_again_as_large(host, tmp_path):
    """Inter frames on; key, inter, dropped and duplicate records; every fresh curve 1.5 x its record, so fresh / recorded leaves
    1.0; the file's one key frame is the first, so that class has Tot <= Seen from then on and leaves nothing."""
    types = [TP.KEY, TP.INTER, TP.INTER, TP.DUP, TP.DROPPED, TP.INTER, TP.DUP, TP.DUP, TP.INTER, TP.DROPPED, TP.INTER, TP.INTER]
    recs = [dict(type=t, qi=k, bits=8 * k, E=[0] * 64 if t == TP.DUP else [(3000 if t == TP.KEY else 400 + 100 * (k % 3)) * (q + 1)
                                                                       for q in range(64)]) for k, t in enumerate(types)]
    fresh = [[3 * x // 2 for x in r["E"]] for r in recs]
    m, fr = _replayed(host, tmp_path, recs, fresh, 40000, inter=True, K=4)
    assert len(fr) == 9 and [d["key"] for d in fr] == [1] + [0] * 8 and [d["tp_type"] for d in fr] == [t for t in types if t != TP.DUP]
    assert m.c2.seen[0] == m.hdr["tot"][0] and m.c2.seen[1] == m.hdr["tot"][1]
    assert all(d["tp_corr"][2:] == [98304, 98304 if n else 65536] for n, d in enumerate(fr))
    qis = [d["qi"] for d in fr]
    assert 0 < min(qis) and max(qis) < 63 and fr[-1]["recorded_left"] == 0 and fr[0]["recorded_left"] > 0
