"""Resized picture output (thip_picture_resize) without a GPU: the numpy restatement of the definition
(tests/picture_resize_ref.py) against thip_picture_out's restatement where the two must agree, against values worked out by hand,
the float elements bit by bit, the kernel's body run on the host under sanitizers, and the argument checks that return before any
state is touched."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import picture_ref, picture_resize_ref as rr

MEAN_STD = (1 / (255 * 0.229), -0.485 / 0.229)     # scale, bias of (c / 255 - 0.485) / 0.229


def _planes(w, h, fmt, seed):
    hdec, vdec = rr.decs(fmt)
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h >> vdec, w >> hdec), (h >> vdec, w >> hdec))]


@pytest.mark.parametrize("fmt", [0, 2, 3])
@pytest.mark.parametrize("rect", [None, (4, 6, 22, 10), (2, 0, 46, 32)])
def test_own_size_is_picture_out(fmt, rect):
    """At the rectangle's own size bilinear R'G'B' is THIP_CHROMA_LINEAR, area R'G'B' is THIP_CHROMA_NEAREST and "ycbcr" is the
    planes, for whole frames and for rectangles with even corners and sizes (where the chroma of the rectangle pairs up with its
    luma as a frame's does).  The resize clamps at the rectangle, thip_picture_out at the coded plane: the picture the identity
    names is thip_picture_out's of the rectangle's planes."""
    planes = _planes(48, 32, fmt, 5 + fmt)
    src = rr.source_planes(planes, fmt, rect)
    h, w = src[0].shape
    for f in ("rgb", "rgba", "rgb_planar"):
        assert np.array_equal(rr.resize(planes, fmt, (w, h), f, "bilinear", rect), picture_ref.picture(src, fmt, f, "linear")), f
        assert np.array_equal(rr.resize(planes, fmt, (w, h), f, "area", rect), picture_ref.picture(src, fmt, f, "nearest")), f
    if rect is None:      # (a whole frame: nothing is cropped, so thip_picture_out of the frame itself)
        assert np.array_equal(rr.resize(planes, fmt, (w, h), "rgb", "bilinear"), picture_ref.picture(planes, fmt, "rgb", "linear"))
    for filt in ("bilinear", "area"):
        got = rr.resize(planes, fmt, (w, h), "ycbcr", filt, rect)
        assert all(np.array_equal(g, s) for g, s in zip(got, picture_ref.picture(planes, fmt, "ycbcr", rect=rect))), filt


@pytest.mark.parametrize("filt", ["bilinear", "area"])
def test_a_constant_plane_stays_constant(filt):
    for (sw, sh) in ((1, 1), (5, 3), (16, 16), (33, 9)):
        s = np.full((sh, sw), 201, np.uint8)
        for (ow, oh) in ((1, 1), (2, 2), (7, 5), (16, 16), (40, 31), (224, 224)):
            if filt == "area" and (sw > 32 * ow or sh > 32 * oh):
                continue
            assert (rr.FILTERS[filt](s, ow, oh) == 201).all(), (sw, sh, ow, oh)


def test_weights_and_positions_by_hand():
    assert rr.area_weights(4, 2).tolist() == [[2, 2, 0, 0], [0, 0, 2, 2]]
    assert rr.area_weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]            # each row sums to S = 3
    assert rr.area_weights(2, 4).tolist() == [[2, 0], [2, 0], [0, 2], [0, 2]]  # upscaling: nearest neighbour
    for S, O in ((4, 2), (3, 2), (2, 4), (33, 2), (5, 7)):
        assert (rr.area_weights(S, O).sum(1) == S).all()
    # 2 -> 4 bilinear: centres at -0.25, 0.25, 0.75, 1.25 source samples, clamped to [0, 1]: Q8 positions 0, 64, 192, 256
    i0, i1, f = rr.bilinear_positions(2, 4)
    assert (i0 * 256 + f).tolist() == [0, 64, 192, 256]
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0, 64, 192, 0]
    # 4 -> 2: centres at 0.5 and 2.5; 1 -> 3: every position clamps to the one sample
    i0, i1, f = rr.bilinear_positions(4, 2)
    assert (i0.tolist(), i1.tolist(), f.tolist()) == ([0, 2], [1, 3], [128, 128])
    i0, i1, f = rr.bilinear_positions(1, 3)
    assert (i0.tolist(), i1.tolist(), f.tolist()) == ([0, 0, 0], [0, 0, 0], [0, 0, 0])


def test_area_by_taps_is_area_by_weight_matrices():
    rng = np.random.default_rng(4)
    for (sw, sh) in ((1, 1), (5, 3), (33, 9), (64, 47), (100, 30)):
        s = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        for (ow, oh) in ((2, 1), (4, 2), (5, 3), (17, 33), (64, 64), (99, 31)):
            if sw <= 32 * ow and sh <= 32 * oh:
                assert np.array_equal(rr.area(s, ow, oh), rr.area_dense(s, ow, oh)), (sw, sh, ow, oh)


def test_area_of_a_ramp_by_hand():
    """5 x 3 -> 2 x 2 with Python integers: columns weigh [2, 2, 1, 0, 0] and [0, 0, 1, 2, 2], rows [2, 1, 0] and [0, 1, 2]."""
    s = [[10 * j + i for i in range(5)] for j in range(3)]
    wx = [[2, 2, 1, 0, 0], [0, 0, 1, 2, 2]]
    wy = [[2, 1, 0], [0, 1, 2]]
    want = [[(sum(wy[Y][j] * wx[X][i] * s[j][i] for j in range(3) for i in range(5)) + (15 >> 1)) // 15 for X in range(2)]
            for Y in range(2)]
    assert want == [[4, 7], [17, 20]]        # the sums are 62, 98, 262 and 298: (sum + 7) // 15
    assert rr.area(np.array(s, np.uint8), 2, 2).tolist() == want


def test_chroma_to_luma_size_is_chroma_linear():
    """4:2:0 chroma taken to the luma size by the bilinear filter is exactly THIP_CHROMA_LINEAR's (9a + 3b + 3c + d + 8) >> 4."""
    c = np.random.default_rng(9).integers(0, 256, (12, 20), dtype=np.uint8)
    assert np.array_equal(rr.bilinear(c, 40, 24), picture_ref.upsample(c, 40, 24, 1, 1, "linear"))
    assert np.array_equal(rr.area(c, 40, 24), picture_ref.upsample(c, 40, 24, 1, 1, "nearest"))


def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _round_f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]      # a Python float (binary64) rounded to binary32, nearest even


def test_float_elements_bit_by_bit():
    """Over all 256 inputs: float32 equals a scalar restatement in which struct rounds a binary64 product, then a binary64 sum,
    to binary32 (the product of two binary32 values is exact in binary64, and so is the sum at these magnitudes, so each is
    rounded once); float16 is that value packed as 'e'."""
    scale, bias = _round_f32(MEAN_STD[0]), _round_f32(MEAN_STD[1])
    c = np.arange(256, dtype=np.uint8)
    f32 = rr.normalise(c, scale, bias, np.float32)
    f16 = rr.normalise(c, scale, bias, np.float16)
    assert f32.dtype == np.float32 and f16.dtype == np.float16
    for k in range(256):
        v = _round_f32(_round_f32(float(k) * scale) + bias)
        assert int(f32.view(np.uint32)[k]) == _f32_bits(v), k
        assert int(f16.view(np.uint16)[k]) == struct.unpack("<H", struct.pack("<e", v))[0], k
    planes = _planes(16, 16, 0, 1)
    out = rr.resize(planes, 0, (7, 5), "rgb_planar", "area", None, np.float16, [scale] * 3, [bias] * 3)
    u8 = rr.resize(planes, 0, (7, 5), "rgb_planar", "area")
    assert out.dtype == np.float16 and np.array_equal(out.view(np.uint16), f16.view(np.uint16)[u8])


def test_kernel_body_on_the_host_stays_inside_its_rectangles(tmp_path):
    """k_picture_resize's lanes run one by one on the host under AddressSanitizer and UBSan (tests/native/picture_resize_host.cpp):
    no load leaves the source rectangle, no store leaves its destination rectangle, every 16-byte store is aligned, and the output
    equals a plain restatement of the definition -- four formats, three pixel formats, both filters, rectangles and outputs around
    the 16-sample chunk, offsets 0..2, tight and padded rows, aligned and odd bases, uint8 and for the planar format both floats.
    The six (format, element) pairs run side by side."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "picture_resize_host")
    cmd = ["g++", "-std=c++17", "-O0", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused",
           "-I" + os.path.join(root, "theora_amd", "csrc"), os.path.join(root, "tests", "native", "picture_resize_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    procs = [subprocess.Popen([exe, str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in range(6)]
    for k, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        # 3 pixel formats x 2 filters x 24 rectangles x 3 offsets x 18 output sizes x 4 destinations = 31104, of which the 432 with
        # a 33-wide rectangle, an output one wide and the area filter are beyond its limit
        assert p.returncode == 0 and out.startswith("ok: 30672 cases, 432 beyond the area limit"), (k, out[-500:], err[-3000:])


def _req(**kw):
    from theora_amd import _lib
    r = _lib.PictureResizeReq()
    r.state, r.bufi = None, -1
    r.format, r.filter, r.elem = _lib.PIC_RGB_PLANAR, _lib.FILTER_AREA, _lib.ELEM_U8
    r.out_width, r.out_height = 17, 9
    for p in range(3):
        r.dst[p], r.dst_pitch[p] = 0x1000, 17           # never dereferenced: every case below is refused
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_picture_resize_arguments_checked_without_a_state():
    from theora_amd import _lib
    L = _lib.load()
    good = _req()
    assert L.thip_picture_resize(None, 1, None) == _lib.EFAULT
    assert L.thip_picture_resize(None, 0, None) == _lib.OK
    assert L.thip_picture_resize(C.byref(good), 0, None) == _lib.OK
    assert L.thip_picture_resize(C.byref(good), -1, None) == _lib.EINVAL
    assert L.thip_picture_resize(C.byref(good), 1, None) == _lib.EFAULT       # a NULL state
    reqs = (_lib.PictureResizeReq * 10)(*([good] * 10))
    assert L.thip_picture_resize(reqs, 10, None) == _lib.EFAULT
    assert C.sizeof(_lib.PictureResizeReq) == 8 + 4 * 10 + 4 * 6 + 3 * 8 + 3 * 8      # (no padding: the header's layout)


def test_shapes_are_the_encoders_planes():
    import theora_amd
    from tests import picture_in_ref
    for fmt in (0, 2, 3):
        for (w, h) in ((96, 80), (17, 33), (1, 1), (224, 224)):
            assert theora_amd.picture_resize_shapes("ycbcr", w, h, fmt) == picture_in_ref.plane_shapes(w, h, fmt, 0, 0)
            assert [(oh, ow) for ow, oh in rr.output_sizes("ycbcr", w, h, fmt)] == picture_in_ref.plane_shapes(w, h, fmt, 0, 0)
    assert theora_amd.picture_resize_shapes("rgb_planar", 224, 200) == (3, 200, 224)
    assert theora_amd.picture_resize_shapes("rgba", 5, 4) == (4, 5, 4)
