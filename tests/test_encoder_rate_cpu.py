"""th_encode_* bitrate mode without a GPU: the control calls of include/theoraenc_hip.h ("Bitrate mode") and the info header's NOMBR
field, which never reach the first frame; and the controller itself (theora_amd/csrc/thip_ratectl.h's RateCtl), replayed on
synthetic probes by tests/native/ratectl_host.cpp under AddressSanitizer and UBSan and compared field by field, exactly, with
tests/enc_rate_ref.py's Controller (tests/ratectl_host.py)."""
import ctypes as C

import pytest

from tests import enc_ref
from tests import ratectl_host as RH


def _enc(**kw):
    from theora_amd import _lib as Lm
    from theora_amd.encoder import Encoder
    return Lm, Encoder(64, 48, 0, 32, **kw)


def _ctl(e, req, val, ctype=C.c_int, size=None, buf=True):
    v = ctype(val)
    rc = e._L.th_encode_ctl(e._enc, req, C.byref(v) if buf else None, C.sizeof(v) if size is None else size)
    return rc, v.value


def test_set_bitrate_sizes_and_values():
    from theora_amd import encoder as E
    Lm, e = _enc()
    try:
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 100000, C.c_int16)[0] == Lm.EINVAL
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 100000, C.c_long, size=3)[0] == Lm.EINVAL
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 100000, buf=False)[0] == Lm.EINVAL
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, -1, C.c_long)[0] == Lm.EINVAL
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, -5, C.c_int)[0] == Lm.EINVAL
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 0, C.c_long)[0] == Lm.EIMPL
        # still quality mode: the rate requests and the stats answer as before
        assert _ctl(e, E.TH_ENCCTL_SET_RATE_FLAGS, 1)[0] == Lm.EIMPL
        assert _ctl(e, E.TH_ENCCTL_SET_QUALITY, 20) == (0, 20)
        assert _ctl(e, E.TH_ENCCTL_THIP_GET_RATE_STATS, 0)[0] == Lm.EINVAL
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 200000, C.c_int)[0] == 0       # an int
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 300000, C.c_long)[0] == 0      # a long, again: a new target
        assert _ctl(e, E.TH_ENCCTL_SET_BITRATE, 0, C.c_long)[0] == Lm.EIMPL    # leaving bitrate mode
        assert _ctl(e, E.TH_ENCCTL_SET_QUALITY, 20)[0] == Lm.EINVAL            # quality is the controller's
    finally:
        e.close()


def test_rate_requests_outside_bitrate_mode_stay_eimpl():
    from theora_amd import encoder as E
    Lm, e = _enc()
    try:
        for req in (E.TH_ENCCTL_SET_RATE_FLAGS, E.TH_ENCCTL_SET_RATE_BUFFER, 24, 26):
            assert _ctl(e, req, 12)[0] == Lm.EIMPL, req
        assert _ctl(e, 0x7299, 0)[0] == Lm.EIMPL
        e.set_bitrate(100000)
        for req in (24, 26, 0x7299):
            assert _ctl(e, req, 0)[0] == Lm.EIMPL, req
    finally:
        e.close()


@pytest.mark.parametrize("asked,got", [(0, 12), (-3, 12), (11, 12), (12, 12), (30, 30), (256, 256), (257, 256), (1 << 30, 256)])
def test_rate_buffer_clamped_and_written_back(asked, got):
    from theora_amd import encoder as E
    Lm, e = _enc(bitrate=100000)
    try:
        assert _ctl(e, E.TH_ENCCTL_SET_RATE_BUFFER, asked) == (0, got)
        assert _ctl(e, E.TH_ENCCTL_SET_RATE_BUFFER, asked, C.c_long)[0] == Lm.EINVAL
    finally:
        e.close()
    _, e = _enc(bitrate=100000, rate_buffer=asked)
    assert e.rate_buffer == got
    e.close()


def test_rate_flags():
    from theora_amd import encoder as E
    Lm, e = _enc(bitrate=64000)
    try:
        for f in (0, 1, 2, 4, 7, E.TH_RATECTL_DROP_FRAMES | E.TH_RATECTL_CAP_UNDERFLOW):
            assert _ctl(e, E.TH_ENCCTL_SET_RATE_FLAGS, f)[0] == 0
        assert _ctl(e, E.TH_ENCCTL_SET_RATE_FLAGS, 1, C.c_int64)[0] == Lm.EINVAL
        # the stats exist in bitrate mode (all zero before the first packet)
        st = e.rate_stats()
        assert st["qi"] == 0 and st["probe"] == [0] * 64
    finally:
        e.close()
    with pytest.raises(ValueError):
        _enc(rate_flags=1)


def _nombr(hdr):
    """The info header's NOMBR field (spec 6.2)."""
    br = enc_ref.BitReader(hdr)
    for nb in [8] * 7 + [8, 8, 8, 16, 16, 24, 24, 8, 8, 32, 32, 24, 24, 8]:
        br.read(nb)
    return br.read(24), br.read(6)


@pytest.mark.parametrize("bitrate,field", [(None, 0), (1, 1), (500000, 500000), ((1 << 24) - 1, (1 << 24) - 1),
                                           (1 << 24, (1 << 24) - 1), (1 << 40, (1 << 24) - 1)])
def test_nombr_field(bitrate, field):
    _, e = _enc(bitrate=bitrate)
    try:
        assert _nombr(e.header_packets()[0]) == (field, 32)
    finally:
        e.close()


def test_nombr_after_headers_stays_zero():
    _, e = _enc()
    try:
        hdr = e.header_packets()
        e.set_bitrate(400000)
        assert _nombr(hdr[0]) == (0, 32)
    finally:
        e.close()


# ---- the controller, replayed on the host (tests/ratectl_host.py) -------------------------------------------------------------------
EASY, HARD = [500 * (q + 1) for q in range(64)], [3000 * (q + 1) for q in range(64)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return RH.build(tmp_path_factory)


def _frames(got):
    return [d for step, d in got if step == "frame"]


def test_controller_intra_only(host, tmp_path):
    """Intra-only, the default buffer and flags, A = E[qi]: easy and hard curves in turn."""
    m = RH.Model()
    m.bitrate(30 * 40000)
    qis = [m.frame(HARD if f % 2 else EASY) for f in range(40)]
    fr = _frames(m.run(host, tmp_path))
    assert all(d["D"] == 12 and d["T"] == 40000 and d["key"] == 1 for d in fr)
    assert [d["qi"] for d in fr] == qis and len(set(qis)) > 2


def test_controller_inter_frames(host, tmp_path):
    """K = 30 and no explicit buffer (D = 30); 70 frames: the look-ahead's count of key and inter frames crosses two key positions.
    A = 2 E[qi]: both corrections move."""
    m = RH.Model(inter=True, K=30)
    m.bitrate(30 * 60000)
    for f in range(70):
        m.frame(HARD if f % 30 == 0 else EASY, mul=2)
    fr = _frames(m.run(host, tmp_path))
    assert all(d["D"] == 30 for d in fr) and [f for f, d in enumerate(fr) if d["key"]] == [0, 30, 60]
    assert fr[0]["c"][0] > 65536 and fr[0]["c"][1] == 65536 and fr[-1]["c"][0] > 65536 and fr[-1]["c"][1] > 65536


def test_controller_drops(host, tmp_path):
    """Curves whose E[0] no frame's share pays for: frames are dropped -- but never the first, and not where a duplicate's granule
    would not fit (offset from the key frame plus the frame's own duplicates reaches 1 << 2).  A duplicate before the controller has
    started is nothing."""
    m = RH.Model(inter=True, K=4, shift=2)
    m.bitrate(30 * 10000)
    m.dup()
    big = [200000 + 1000 * q for q in range(64)]
    out = []
    for f in range(16):
        dups = 1 if f % 5 == 1 else 0
        out.append(m.frame(big, dups=dups))
        for _ in range(dups):
            m.dup()
    got = m.run(host, tmp_path)
    assert got[1][0] == "dup" and got[1][1]["started"] == 0 and got[1][1]["cur"] == -1
    fr = _frames(got)
    assert out[0] >= 0 and fr[0]["dropped"] == 0
    starved = [d for d in fr[1:] if d["fullness_before"] + d["target"] - d["estimate"] < 0 and d["qi"] == 0 or d["dropped"]]
    assert any(d["dropped"] for d in starved) and any(not d["dropped"] for d in starved)   # both sides of the granule rule
    assert any(d["duplicate"] for step, d in got if step == "dup")


@pytest.mark.parametrize("flags", [0, RH.RR.CAP_UNDERFLOW, 7])
def test_controller_flags(host, tmp_path, flags):
    """Packets far below T, then far above: with a cap off F leaves [0, R] on that side, with it on the cap binds."""
    m = RH.Model()
    m.bitrate(30 * 40000)
    m.flags(flags)
    tiny = [8 + q for q in range(64)]
    for f in range(30):
        m.frame(tiny, mul=0, add=8 if f < 20 else 20 * 40000)
    fr = _frames(m.run(host, tmp_path))
    assert not any(d["dropped"] for d in fr)
    free = [d["fullness_before"] + d["target"] - d["actual"] for d in fr]   # F before the caps
    under = [d for d, x in zip(fr, free) if x < 0]
    over = [d for d, x in zip(fr, free) if x > d["R"]]
    assert under and over
    if flags & RH.RR.CAP_UNDERFLOW:
        assert all(d["fullness_after"] == 0 for d in under)
    else:
        assert all(d["fullness_after"] < 0 for d in under)
    if flags & RH.RR.CAP_OVERFLOW:
        assert all(d["fullness_after"] == d["R"] for d in over)
    else:
        assert all(d["fullness_after"] > d["R"] for d in over)


def test_controller_retarget_and_rebuffer(host, tmp_path):
    """TH_ENCCTL_SET_BITRATE and TH_ENCCTL_SET_RATE_BUFFER before the start (settings only) and mid-stream (T, R, F* anew and
    F = min(F, R))."""
    m = RH.Model(inter=True, K=16)
    m.bitrate(30 * 10000)
    m.buffer(300)
    m.bitrate(30 * 40000)
    m.flags(0)
    for f in range(8):
        m.frame(EASY, mul=0, add=8)          # F grows
    m.bitrate(30 * 20000)
    m.frame(EASY)
    m.buffer(5)
    for f in range(8):
        m.frame(EASY)
    got = m.run(host, tmp_path)
    assert [d["started"] for _, d in got[:4]] == [0] * 4 and got[1][1]["buf"] == 256
    re = [d for step, d in got if step in ("bitrate", "buffer") and d["started"]]
    assert [(d["T"], d["D"]) for d in re] == [(20000, 256), (20000, 12)] and all(d["F"] == d["R"] == 2 * d["Fstar"] for d in re)


def test_controller_with_one_frame_type_seen(host, tmp_path):
    """K = 4, D = 12, S = 12 T = 480000 at the first frame.  A key frame first (HARD, 3000 (q + 1)): 2 key and 9 inter frames follow,
    the inter term is the key term / 4: 3000 + 2 x 3000 + 9 x 750 = 15750 a step, qi 29.  An inter frame first (EASY, 500 (q + 1);
    the encoder never does this, the controller takes it): the key position is -1, 3 key and 8 inter frames follow, the key term is
    4 x the inter term: 500 + 3 x 2000 + 8 x 500 = 10500 a step, qi 44."""
    for key, curve, qi in ((True, HARD, 29), (False, EASY, 44)):
        m = RH.Model(inter=True, K=4)
        m.bitrate(30 * 40000)
        assert m.frame(curve, key=key) == qi
        assert _frames(m.run(host, tmp_path))[0]["qi"] == qi


@pytest.mark.parametrize("bitrate,T", [(1, 32), (1 << 46, 1 << 40)])
def test_controller_extremes(host, tmp_path, bitrate, T):
    """T at both ends of its clamp with D = 256, probe entries up to 2^32 - 1 and packets of 2^40 bits (c reaches its cap 2^20:
    Cur(q) up to 2^52, Future(q) up to 2^62), and a stream of which the controller has seen one frame type only: the inter term is
    the key term / 4, and (the first frame taken as an inter frame, which the encoder never does) the key term 4 x the inter term."""
    top = [(1 << 32) - 1 - 1000 * (63 - q) for q in range(64)]
    for first_key in (True, False):
        m = RH.Model(inter=True, K=64)
        m.bitrate(bitrate)
        m.buffer(256)
        m.flags(0)
        for f in range(12):
            m.frame(top, mul=0, add=1 << 40, key=first_key if f == 0 else None)
        for f in range(4):
            m.frame(top, mul=1)
        fr = _frames(m.run(host, tmp_path))
        assert all(d["T"] == T and d["D"] == 256 for d in fr) and fr[0]["key"] == int(first_key)
        assert max(max(d["c"]) for d in fr) == 1 << 20 and max(d["estimate"] for d in fr) >= 16 * top[0]   # (E c >> 16 at the cap)
