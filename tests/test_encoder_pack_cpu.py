"""th_encode_*'s device packetiser without a GPU: the two controls (TH_ENCCTL_THIP_SET_DEVICE_PACK, TH_ENCCTL_THIP_GET_PACK_STATS),
the statistics' layout, the run-time option that sets a context's initial state, and the Python face.  Nothing here reaches the first
th_encode_ycbcr_in, so nothing touches the GPU (this machine may have none)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH_EINVAL, TH_EIMPL = -10, -23


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
    assert (E.TH_ENCCTL_THIP_SET_DEVICE_PACK, E.TH_ENCCTL_THIP_GET_PACK_STATS) == (0x720D, 0x720E)
    for name in ("TH_ENCCTL_THIP_SET_DEVICE_PACK", "TH_ENCCTL_THIP_GET_PACK_STATS"):
        m = re.search(r"#define %s \((0x[0-9A-Fa-f]+)\)" % name, hdr)
        assert m and int(m.group(1), 16) == getattr(E, name), name
    body = re.search(r"typedef struct thip_enc_pack_stats \{(.*?)\} thip_enc_pack_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(int32_t|int64_t|double)\s+(\w+);", body)]
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(E.PackStats._fields_)
    assert C.sizeof(E.PackStats) == 40
    assert "Device packetiser" in hdr


def test_device_pack_controls():
    """0 and 1 accepted, anything else TH_EINVAL; the statistics before any packet are all zero; 0x7299 is still unknown."""
    from theora_amd import encoder as E
    L, enc = _enc()
    try:
        for v in (1, 0, 1, 1, 0):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_DEVICE_PACK, v) == (0, v)
        for v in (2, -1, 3, 1 << 20, -(1 << 31)):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_DEVICE_PACK, v)[0] == TH_EINVAL, v
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_DEVICE_PACK, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_DEVICE_PACK, 1, C.c_int64)[0] == TH_EINVAL
        s = E.PackStats()
        C.memset(C.byref(s), 0xFF, C.sizeof(s))
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_PACK_STATS, C.byref(s), C.sizeof(s)) == 0
        assert bytes(s) == bytes(C.sizeof(s))
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_PACK_STATS, C.byref(s), C.sizeof(s) - 4) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_PACK_STATS, None, C.sizeof(s)) == TH_EINVAL
        # with the other switches on as well, and after them
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, 5) == (0, 5)
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_DEVICE_PACK, 1) == (0, 1)
        assert _ctl(L, enc, 0x7299, 0)[0] == TH_EIMPL   # (still pinned)
    finally:
        L.th_encode_free(enc)


def test_option_sets_the_initial_state_and_is_documented():
    from theora_amd import _lib
    L = _lib.load()
    v = C.c_int(12345)
    assert L.thip_get_option(b"enc_device_pack", C.byref(v)) == 0
    if "THIP_ENC_DEVICE_PACK" not in os.environ:
        assert v.value == 0
    assert L.thip_get_option(b"enc_pack_cap", C.byref(v)) == 0
    if "THIP_ENC_PACK_CAP" not in os.environ:
        assert v.value == 0
    hdr = open(os.path.join(ROOT, "include", "theora_hip.h")).read()
    assert " enc_device_pack" in hdr and "THIP_ENC_DEVICE_PACK" in hdr and " enc_pack_cap" in hdr
    # a context made while the option is set starts with the packetiser on: nothing to see without a frame, but it must not fail
    before = L.thip_option(b"enc_device_pack")
    try:
        assert L.thip_set_option(b"enc_device_pack", 1) == 0
        Lx, enc = _enc()
        Lx.th_encode_free(enc)
    finally:
        L.thip_set_option(b"enc_device_pack", before)


def test_python_encoder_device_pack():
    from theora_amd.encoder import Encoder
    for dp in (None, False, True):
        e = Encoder(64, 48, 0, 20, device_pack=dp)
        assert e.pack_stats() == dict(device=0, phase=0, header_bits=0, token_bits=0, pack_ms=0.0, fallbacks=0)
        e.set_device_pack(True)
        e.set_device_pack(False)
        e.close()
    assert Encoder(64, 48, 0, 20).header_packets() == Encoder(64, 48, 0, 20, device_pack=True).header_packets()
