"""th_encode_*'s inter-frame controls without a GPU (TH_ENCCTL_THIP_SET_INTER_FRAMES and its neighbours), and the restatement's
own building blocks (tests/enc_inter_ref.py).  Nothing here reaches the first th_encode_ycbcr_in."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_inter_ref as R

TH_EINVAL, TH_EIMPL = -10, -23


def _enc(**kw):
    from theora_amd import _lib
    from theora_amd.encoder import make_info
    L = _lib.load()
    info = make_info(64, 48, 0, 32, kfgshift=kw.pop("kfgshift", 6))
    enc = L.th_encode_alloc(C.byref(info))
    assert enc
    return L, enc


def _ctl(L, enc, req, value, ctype=C.c_int):
    v = ctype(value)
    return L.th_encode_ctl(enc, req, C.byref(v), C.sizeof(v)), v.value


def test_inter_controls_are_known():
    from theora_amd import encoder as E
    L, enc = _enc()
    try:
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1) == (0, 1)
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 0) == (0, 0)
        assert _ctl(L, enc, 0x7299, 0)[0] == TH_EIMPL
        s = E.InterStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_INTER_STATS, C.byref(s), C.sizeof(s)) == 0
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_INTER_STATS, C.byref(s), C.sizeof(s) - 4) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, None, 4) == TH_EINVAL
    finally:
        L.th_encode_free(enc)


@pytest.mark.parametrize("shift", [0, 3, 6])
def test_keyframe_interval_is_clamped_with_inter_frames(shift):
    from theora_amd import encoder as E
    L, enc = _enc(kfgshift=shift)
    try:
        # off: exactly what the intra-only encoder answers
        assert _ctl(L, enc, E.TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE, 12, C.c_uint32) == (0, 1)
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        for want, got in ((12, min(12, 1 << shift)), (0, 1), (1, 1), (1 << 20, 1 << shift), (0xFFFFFFFF, 1 << shift)):
            assert _ctl(L, enc, E.TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE, want, C.c_uint32) == (0, got)
    finally:
        L.th_encode_free(enc)


def test_get_recon_needs_inter_frames_and_a_frame():
    from theora_amd import encoder as E
    from theora_amd._lib import ThImgPlane
    L, enc = _enc()
    try:
        planes = [np.zeros((48, 64), np.uint8)] + [np.zeros((24, 32), np.uint8)] * 2
        buf = (ThImgPlane * 3)()
        for p in range(3):
            buf[p].width, buf[p].height, buf[p].stride = planes[p].shape[1], planes[p].shape[0], planes[p].strides[0]
            buf[p].data = planes[p].ctypes.data_as(C.POINTER(C.c_ubyte))
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RECON, buf, C.sizeof(buf)) == TH_EINVAL   # off
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RECON, buf, C.sizeof(buf)) == TH_EINVAL   # no frame yet
    finally:
        L.th_encode_free(enc)


def test_headers_do_not_change_with_inter_frames():
    from theora_amd.encoder import Encoder
    a = Encoder(64, 48, 0, 20).header_packets()
    b = Encoder(64, 48, 0, 20, inter=True, keyframe_interval=8).header_packets()
    assert a == b


def test_python_encoder_interval():
    from theora_amd.encoder import Encoder
    assert Encoder(64, 48, 0, 20, kfgshift=3, inter=True).keyframe_interval == 8
    assert Encoder(64, 48, 0, 20, kfgshift=3, inter=True, keyframe_interval=100).keyframe_interval == 8
    assert Encoder(64, 48, 0, 20, kfgshift=0, inter=True, keyframe_interval=4).keyframe_interval == 1
    with pytest.raises(ValueError):
        Encoder(64, 48, 0, 20, keyframe_interval=4)


def test_mv_axis_matches_the_decoders_offsets():
    """The restatement's mv_axis against the oracle's offsets (oc_state_get_mv_offsets) for every luma and chroma component."""
    import oracle
    stride = 1000
    for q in (False, True):
        for v in range(-31, 32):
            w, f = R.mv_axis(v, q)
            n, o0, o1 = oracle.mv_offsets(stride, int(q), 0, v, 0)
            offs = {int(w)} | ({int(w + f)} if f else set())
            assert offs == ({o0, o1} if n == 2 else {o0}), (q, v, n, o0, o1, offs)


def test_motion_search_finds_a_pan():
    rng = np.random.default_rng(1)
    ref = rng.integers(0, 256, (64, 96)).astype(np.uint8)
    src = np.pad(ref, 8, mode="edge")[8 + 3:8 + 3 + 64, 8 - 5:8 - 5 + 96]   # src(x, y) = ref(x - 5, y + 3)
    mode, mvx, mvy = R.motion_search(src, ref, 20)[:3]
    inner = [r * 6 + c for r in range(1, 3) for c in range(1, 5)]
    assert (mode[inner] == R.MV).all()
    assert (mvx[inner] == -10).all() and (mvy[inner] == 6).all()
