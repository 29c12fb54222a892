"""R'G'B' picture input (thip_picture_in, TH_ENCCTL_THIP_RGB_IN) without a GPU: the numpy restatement of the definition
(tests/picture_in_ref.py) against the specification's real-valued formula and against thip_picture_out's matrix, the geometry
against the encoder's chroma region, and the argument checks that return before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_ref, picture_in_ref, picture_ref

# |integer - real-valued formula|: 0.5 of rounding + 3 * 255 * 0.5 / 65536 of rounded coefficients < 0.506
BOUND = 0.51


def _all_colours():
    """Every (R, G, B), one 2^16 slab of G, B per R."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    for r in range(256):
        yield np.full_like(g, r), g, b


def test_all_colours_range_spec_distance_and_round_trip():
    lo, hi = [255] * 3, [0] * 3
    worst, back = 0.0, [0, 0, 0]
    for R, G, B in _all_colours():
        Y = picture_in_ref.luma(R, G, B)
        Cb, Cr = picture_in_ref.chroma(R, G, B, 0)
        for k, p in enumerate((Y, Cb, Cr)):
            lo[k], hi[k] = min(lo[k], int(p.min())), max(hi[k], int(p.max()))
        for got, want in zip((Y, Cb, Cr), picture_in_ref.spec_ycbcr(R, G, B)):
            worst = max(worst, float(np.abs(got - want).max()))
        for k, (c0, c1) in enumerate(zip((R, G, B), picture_ref.ycbcr_to_rgb(Y, Cb, Cr))):
            back[k] = max(back[k], int(np.abs(c1.astype(np.int32) - c0).max()))
    assert (lo, hi) == ([16, 16, 16], [235, 240, 240])     # no clamp anywhere
    assert worst < BOUND, worst
    assert back[0] <= 1 and back[1] <= 1 and back[2] <= 2, back


@pytest.mark.parametrize("s", [1, 2])
def test_mean_of_a_group_is_within_the_bound_of_the_formula_on_the_real_mean(s):
    rng = np.random.default_rng(40 + s)
    px = rng.integers(0, 256, (2_000_000, 1 << s, 3), dtype=np.int32)
    px[:1000] = rng.integers(0, 2, (1000, 1 << s, 3)) * 255          # saturated corners, mixed
    S = px.sum(1)
    Cb, Cr = picture_in_ref.chroma(S[:, 0], S[:, 1], S[:, 2], s)
    mean = S / float(1 << s)
    _, wb, wr = picture_in_ref.spec_ycbcr(mean[:, 0], mean[:, 1], mean[:, 2])
    assert float(np.abs(Cb - wb).max()) < BOUND and float(np.abs(Cr - wr).max()) < BOUND
    assert Cb.min() >= 16 and Cb.max() <= 240 and Cr.min() >= 16 and Cr.max() <= 240


GEOMETRY = [   # (pic_x, pic_y, width, height)
    (0, 0, 1, 1), (1, 1, 1, 1), (1, 1, 2, 2), (3, 5, 17, 9), (0, 1, 33, 18), (2, 4, 16, 16), (1, 0, 16, 15), (0, 0, 176, 144),
    (1, 2, 61, 45), (5, 3, 40, 41)]


@pytest.mark.parametrize("fmt", [0, 2, 3])
@pytest.mark.parametrize("px,py,w,h", GEOMETRY)
def test_plane_shapes_are_the_encoders_region_and_grey_stays_grey(px, py, w, h, fmt):
    import theora_amd
    shapes = picture_in_ref.plane_shapes(w, h, fmt, px, py)
    assert shapes == theora_amd.picture_in_shapes(w, h, fmt, px, py)
    for p in range(3):
        x0, y0, cw, ch = enc_ref.chroma_region((px, py, w, h), fmt, p)     # the encoder's cx0 / cy0 / cw / ch, restated
        assert shapes[p] == (ch, cw), p
    rng = np.random.default_rng(px + 7 * w + fmt)
    grey = np.repeat(rng.integers(0, 256, (h, w, 1), dtype=np.uint8), 3, 2)
    Y, Cb, Cr = picture_in_ref.picture_in(grey, fmt, "rgb", px, py)
    assert [p.shape for p in (Y, Cb, Cr)] == shapes
    assert (Cb == 128).all() and (Cr == 128).all()
    assert np.array_equal(Y, picture_in_ref.luma(grey[..., 0], grey[..., 0], grey[..., 0]))


def test_pairing_by_hand():
    """Odd offsets shift the pairing: at pic_x = 1 the first chroma column is pixel 0 twice, the second pixels 1 and 2."""
    img = np.zeros((2, 4, 3), np.uint8)
    img[..., 2] = [[0, 40, 80, 120], [200, 240, 16, 56]]                  # blue only
    _, cb, _ = picture_in_ref.picture_in(img, 2, "rgb", pic_x=1)          # 4:2:2
    want = [[(0, 0), (40, 80), (120, 120)], [(200, 200), (240, 16), (56, 56)]]
    assert cb.shape == (2, 3)
    for j in range(2):
        for i in range(3):
            assert cb[j, i] == 128 + ((28784 * sum(want[j][i]) + (1 << 16)) >> 17)
    _, cb, _ = picture_in_ref.picture_in(img, 0, "rgb", pic_x=0, pic_y=1)  # 4:2:0: row 0 alone, then row 1 alone
    assert cb.shape == (2, 2)
    assert cb[0, 1] == 128 + ((28784 * 2 * (80 + 120) + (1 << 17)) >> 18)
    assert cb[1, 0] == 128 + ((28784 * 2 * (200 + 240) + (1 << 17)) >> 18)
    # the three formats carry the same picture
    rgba = np.concatenate([img, np.full((2, 4, 1), 99, np.uint8)], 2)
    planar = np.ascontiguousarray(img.transpose(2, 0, 1))
    a = picture_in_ref.picture_in(img, 0, "rgb", 1, 1)
    for other, f in ((rgba, "rgba"), (planar, "rgb_planar")):
        assert all(np.array_equal(x, y) for x, y in zip(a, picture_in_ref.picture_in(other, 0, f, 1, 1)))


def test_kernel_body_on_the_host_stays_inside_its_rows(tmp_path):
    """k_picture_in's lanes run one by one on the host under AddressSanitizer and UBSan (tests/native/picture_in_host.cpp): no load
    leaves the source row it belongs to, no store leaves its destination rectangle, every 16-byte access is aligned, and the planes
    equal the definition -- three formats, three pixel formats, widths around the 16-pixel chunk, offsets 0..2, tight and padded
    rows, aligned and odd bases."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "picture_in_host")
    cmd = ["g++", "-std=c++17", "-O0", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused",
           "-I" + os.path.join(root, "theora_amd", "csrc"), os.path.join(root, "tests", "native", "picture_in_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok: 10368 cases"), (r.stdout[-500:], r.stderr[-3000:])


def _req(**kw):
    from theora_amd import _lib
    r = _lib.PictureInReq()
    r.format, r.pixel_fmt = _lib.PIC_RGB24, 0
    r.pic_x, r.pic_y, r.width, r.height = 1, 1, 17, 9
    for p in range(3):
        r.src[p], r.src_pitch[p] = 0x1000, 4 * 17          # never dereferenced: every case below is refused
        r.dst[p], r.dst_pitch[p] = 0x1000, 17
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_picture_in_arguments_checked_without_a_device():
    from theora_amd import _lib
    L = _lib.load()
    i64 = C.c_int64 * 3
    ptr = C.c_void_p * 3
    good = _req()
    assert L.thip_picture_in(None, 1, None) == _lib.EFAULT
    assert L.thip_picture_in(None, 0, None) == _lib.OK
    assert L.thip_picture_in(C.byref(good), 0, None) == _lib.OK
    assert L.thip_picture_in(C.byref(good), -1, None) == _lib.EINVAL
    bad = [(_lib.EINVAL, _req(format=_lib.PIC_YCBCR)), (_lib.EINVAL, _req(format=4)), (_lib.EINVAL, _req(format=-1)),
           (_lib.EINVAL, _req(pixel_fmt=1)), (_lib.EINVAL, _req(pixel_fmt=4)), (_lib.EINVAL, _req(pixel_fmt=-1)),
           (_lib.EINVAL, _req(width=0)), (_lib.EINVAL, _req(height=0)), (_lib.EINVAL, _req(width=-3)),
           (_lib.EINVAL, _req(pic_x=-1)), (_lib.EINVAL, _req(pic_y=-2)),
           (_lib.EINVAL, _req(src_pitch=i64(3 * 17 - 1, 0, 0))),
           (_lib.EINVAL, _req(format=_lib.PIC_RGBA32, src_pitch=i64(4 * 17 - 1, 0, 0))),
           (_lib.EINVAL, _req(format=_lib.PIC_RGB_PLANAR, src_pitch=i64(17, 17, 16))),
           (_lib.EINVAL, _req(dst_pitch=i64(16, 17, 17))),
           (_lib.EINVAL, _req(dst_pitch=i64(17, 8, 17))),            # cw = ((1 + 17 + 1) >> 1) - (1 >> 1) = 9
           (_lib.EINVAL, _req(dst_pitch=i64(17, 17, 8))),
           (_lib.EFAULT, _req(src=ptr(None, 0x1000, 0x1000))),
           (_lib.EFAULT, _req(format=_lib.PIC_RGB_PLANAR, src=ptr(0x1000, 0x1000, None))),
           (_lib.EFAULT, _req(dst=ptr(None, 0x1000, 0x1000))), (_lib.EFAULT, _req(dst=ptr(0x1000, 0x1000, None)))]
    for want, r in bad:
        assert L.thip_picture_in(C.byref(r), 1, None) == want
        reqs = (_lib.PictureInReq * 10)(*([good] * 9 + [r]))      # all or nothing: the tenth request stops the first nine
        assert L.thip_picture_in(reqs, 10, None) == want
    assert picture_in_ref.plane_shapes(17, 9, 0, 1, 1)[1] == (5, 9)     # (the cw the pitch cases above are sized by)


def _enc(**kw):
    from theora_amd.encoder import Encoder
    return Encoder(64, 48, kw.pop("fmt", 0), 32, pic=(1, 2, 61, 45), **kw)


def _rgb_in(**kw):
    from theora_amd.encoder import RGB_FORMATS, RgbIn
    a = RgbIn()
    a.format, a.device, a.width, a.height = RGB_FORMATS["rgb"], 0, 61, 45
    for p in range(3):
        a.src[p], a.pitch[p] = 0x1000, 4 * 61
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_rgb_in_ctl_arguments_checked_without_a_device():
    from theora_amd import _lib
    from theora_amd.encoder import RGB_FORMATS, TH_ENCCTL_THIP_RGB_IN
    L = _lib.load()
    e = _enc()
    i64 = C.c_int64 * 3
    ptr = C.c_void_p * 3

    def ctl(a, size=None):
        return L.th_encode_ctl(e._enc, TH_ENCCTL_THIP_RGB_IN, C.byref(a) if a is not None else None, C.sizeof(a) if size is None else size)
    assert L.th_encode_ctl(e._enc, TH_ENCCTL_THIP_RGB_IN, None, 0) == _lib.EFAULT
    assert ctl(_rgb_in(), 8) == _lib.EINVAL
    bad = [(_lib.EINVAL, _rgb_in(format=_lib.PIC_YCBCR)), (_lib.EINVAL, _rgb_in(format=7)),
           (_lib.EINVAL, _rgb_in(device=2)), (_lib.EINVAL, _rgb_in(device=-1)),
           (_lib.EINVAL, _rgb_in(width=64)), (_lib.EINVAL, _rgb_in(height=48)), (_lib.EINVAL, _rgb_in(width=45, height=61)),
           (_lib.EINVAL, _rgb_in(pitch=i64(3 * 61 - 1, 0, 0))),
           (_lib.EINVAL, _rgb_in(format=RGB_FORMATS["rgba"], pitch=i64(4 * 61 - 1, 0, 0))),
           (_lib.EINVAL, _rgb_in(format=RGB_FORMATS["rgb_planar"], pitch=i64(61, 60, 61))),
           (_lib.EFAULT, _rgb_in(src=ptr(None, 0x1000, 0x1000))),
           (_lib.EFAULT, _rgb_in(device=1, src=ptr(None, 0x1000, 0x1000))),
           (_lib.EFAULT, _rgb_in(format=RGB_FORMATS["rgb_planar"], src=ptr(0x1000, None, 0x1000)))]
    for want, a in bad:
        assert ctl(a) == want
    e.close()


def test_encode_rgb_refuses_wrong_pictures_in_python():
    e = _enc()
    with pytest.raises(ValueError):
        e.encode_rgb(np.zeros((45, 61, 3), np.uint8), fmt="bgr")
    with pytest.raises(ValueError):
        e.encode_rgb(np.zeros((45, 61, 4), np.uint8), fmt="rgb")
    with pytest.raises(ValueError):
        e.encode_rgb(np.zeros((45, 61, 3), np.uint8)[:, ::2], fmt="rgb")      # pixels not contiguous
    with pytest.raises(TypeError):
        e.encode_rgb(np.zeros((45, 61, 3), np.float32), fmt="rgb")
    e.close()
