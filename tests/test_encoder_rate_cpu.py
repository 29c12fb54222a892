"""th_encode_* bitrate mode without a GPU: the control calls of include/theoraenc_hip.h ("Bitrate mode") and the info header's NOMBR
field.  Nothing here reaches the first frame."""
import ctypes as C

import pytest

from tests import enc_ref


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
