"""Device-resident pictures (thip_picture_out, TH_DECCTL_THIP_PICTURE_OUT) without a GPU: the numpy restatement of the
definitions against the specification and against hand-computed values, and the argument checks that return before any
device is touched."""
import ctypes as C

import numpy as np

from tests import picture_ref


def test_integer_matrix_is_within_one_lsb_of_the_spec_everywhere():
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for y in range(256):
        got = picture_ref.ycbcr_to_rgb(np.full_like(cb, y), cb, cr)
        want = picture_ref.spec_rgb(np.full_like(cb, y), cb, cr)
        for g, w in zip(got, want):
            worst = max(worst, int(np.abs(g.astype(np.int64) - w).max()))
    assert worst <= 1


def test_integer_matrix_fixed_points():
    R, G, B = picture_ref.ycbcr_to_rgb(np.array([16, 235, 126]), np.array([128, 128, 128]), np.array([128, 128, 128]))
    assert list(R) == [0, 255, 128] and list(G) == [0, 255, 128] and list(B) == [0, 255, 128]


def test_linear_upsampling_420_by_hand():
    c = np.array([[0, 16], [32, 64]])
    up = picture_ref.upsample(c, 4, 4, 1, 1, "linear").astype(int)
    assert up[0, 0] == 0                               # every neighbour clamps onto c[0, 0]
    assert up[0, 1] == (9 * 0 + 3 * 16 + 3 * 0 + 16 + 8) >> 4 == 4
    assert up[1, 1] == (9 * 0 + 3 * 16 + 3 * 32 + 64 + 8) >> 4 == 13
    assert up[1, 2] == (9 * 16 + 3 * 0 + 3 * 64 + 32 + 8) >> 4 == 23
    assert up[3, 3] == 64
    assert np.array_equal(picture_ref.upsample(c, 4, 4, 1, 1, "nearest"), np.repeat(np.repeat(c, 2, 0), 2, 1))


def test_linear_upsampling_422_by_hand():
    c = np.array([[0, 40], [200, 100]])
    up = picture_ref.upsample(c, 4, 2, 1, 0, "linear").astype(int)
    assert list(up[0]) == [0, (0 + 40 + 2) >> 2, (120 + 0 + 2) >> 2, 40] == [0, 10, 30, 40]
    assert list(up[1]) == [200, (600 + 100 + 2) >> 2, (300 + 200 + 2) >> 2, 100]


def test_crop_follows_the_raw_rule():
    planes = [np.arange(16 * 16).reshape(16, 16) % 251, np.arange(64).reshape(8, 8), np.arange(64).reshape(8, 8) + 100]
    out = picture_ref.picture(planes, 0, "ycbcr", rect=(3, 5, 7, 6))
    assert out[0].shape == (6, 7)
    assert np.array_equal(out[1], planes[1][2:6, 1:5])   # rows 5>>1 .. (11+1)>>1, columns 3>>1 .. (10+1)>>1


def test_arguments_checked_without_a_device():
    from theora_amd import _lib
    L = _lib.load()
    req = _lib.PictureReq()
    assert L.thip_picture_out(None, 1, None) == _lib.EFAULT
    assert L.thip_picture_out(None, 0, None) == _lib.OK
    assert L.thip_picture_out(C.byref(req), -1, None) == _lib.EINVAL
    assert L.thip_picture_out(C.byref(req), 1, None) == _lib.EFAULT    # no state


def test_python_shapes():
    import theora_amd
    assert theora_amd.picture_shapes("rgb", 101, 77) == (77, 101, 3)
    assert theora_amd.picture_shapes("rgba", 101, 77) == (77, 101, 4)
    assert theora_amd.picture_shapes("rgb_planar", 101, 77) == (3, 77, 101)
    assert theora_amd.picture_shapes("ycbcr", 101, 77, 3, theora_amd.PF_420, 5) == [(77, 101), (39, 51), (39, 51)]
    assert theora_amd.picture_shapes("ycbcr", 101, 77, 3, theora_amd.PF_422, 5) == [(77, 101), (77, 51), (77, 51)]


def test_decoder_ctls_in_slot_trace_mode():
    """A context without device state: TH_DECCTL_THIP_PICTURE_OUT is TH_EIMPL, TH_DECCTL_THIP_SET_HOST_OUTPUT TH_EINVAL."""
    from theora_amd import _lib
    from theora_amd.decoder import (Decoder, PictureOutArgs, TH_DECCTL_THIP_PICTURE_OUT, TH_DECCTL_THIP_SET_HOST_OUTPUT)
    from tests import streamgen, util
    L = _lib.load()
    with util.options(L, fe_trace_backend=1):
        st = streamgen.Stream(32, 32, 0, 5)
        dec = Decoder(st.header_packets())
        a = PictureOutArgs()
        assert L.th_decode_ctl(dec._dec, TH_DECCTL_THIP_PICTURE_OUT, C.byref(a), C.sizeof(a)) == _lib.EIMPL
        dec.packetin(st.frame(0)[0])
        assert L.th_decode_ctl(dec._dec, TH_DECCTL_THIP_PICTURE_OUT, C.byref(a), C.sizeof(a)) == _lib.EIMPL
        assert L.th_decode_ctl(dec._dec, TH_DECCTL_THIP_PICTURE_OUT, C.byref(a), 3) == _lib.EINVAL
        on = C.c_int(0)
        assert L.th_decode_ctl(dec._dec, TH_DECCTL_THIP_SET_HOST_OUTPUT, C.byref(on), C.sizeof(on)) == _lib.EINVAL
        dec.close()
