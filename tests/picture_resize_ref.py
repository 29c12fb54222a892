"""numpy restatement of thip_picture_resize's definition (include/theora_hip.h), written from the header's text: the source
rectangles, the two filters in integer arithmetic, thip_picture_out's matrix (tests/picture_ref.py) and the float elements.  Planes
are in DISPLAY order (row 0 at the top), the full coded frame, as ycbcr_out() gives them."""
import numpy as np

from tests import picture_ref

AREA_CAP = 32


def decs(pixel_fmt):
    return int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))


def source_planes(planes, pixel_fmt, rect=None):
    """The three rectangles a request reads: thip_picture_out's THIP_PIC_YCBCR planes for the same rectangle."""
    hdec, vdec = decs(pixel_fmt)
    H, W = planes[0].shape
    x, y, w, h = rect if rect is not None else (0, 0, W, H)
    return [planes[0][y:y + h, x:x + w],
            planes[1][y >> vdec:(y + h + vdec) >> vdec, x >> hdec:(x + w + hdec) >> hdec],
            planes[2][y >> vdec:(y + h + vdec) >> vdec, x >> hdec:(x + w + hdec) >> hdec]]


def output_sizes(fmt, out_w, out_h, pixel_fmt):
    """(width, height) each of Y, Cb, Cr is resampled to."""
    if fmt != "ycbcr":
        return [(out_w, out_h)] * 3
    hdec, vdec = decs(pixel_fmt)
    c = ((out_w + hdec) >> hdec, (out_h + vdec) >> vdec)
    return [(out_w, out_h), c, c]


def refused(planes, pixel_fmt, fmt, filt, size, rect=None):
    """True where the area filter's limit refuses the request: a source extent of more than 32 output extents, any plane."""
    if filt != "area":
        return False
    for s, (ow, oh) in zip(source_planes(planes, pixel_fmt, rect), output_sizes(fmt, size[0], size[1], pixel_fmt)):
        if s.shape[1] > AREA_CAP * ow or s.shape[0] > AREA_CAP * oh:
            return True
    return False


def bilinear_positions(S, O):
    """Per output index: (i0, i1, f) of the centre-aligned Q8 position."""
    X = np.arange(O, dtype=np.int64)
    p = ((2 * X + 1) * S - O) * 128 // O          # numpy's // on int64 is a floor division
    p = np.clip(p, 0, (S - 1) * 256)
    i0 = p >> 8
    return i0, np.minimum(i0 + 1, S - 1), p & 255


def bilinear(s, ow, oh):
    s = np.asarray(s, np.int64)
    sh, sw = s.shape
    x0, x1, fx = bilinear_positions(sw, ow)
    y0, y1, fy = bilinear_positions(sh, oh)
    fy = fy[:, None]
    top = (256 - fx) * s[y0][:, x0] + fx * s[y0][:, x1]
    bot = (256 - fx) * s[y1][:, x0] + fx * s[y1][:, x1]
    return (((256 - fy) * top + fy * bot + 32768) >> 16).astype(np.uint8)


def area_weights(S, O):
    """(O, S) integer matrix: row X holds the overlap of [X S, (X + 1) S) with each [i O, (i + 1) O)."""
    X = np.arange(O, dtype=np.int64)[:, None]
    i = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((X + 1) * S, (i + 1) * O) - np.maximum(X * S, i * O), 0)


def _area_axis(a, S, O):
    """sum_i w[X][i] a[..., i] along the last axis without the dense matrix: output X overlaps the samples from X S // O on, at
    most S // O + 2 of them; the overlap of the others is empty."""
    X = np.arange(O, dtype=np.int64)
    out = np.zeros(a.shape[:-1] + (O,), np.int64)
    for t in range(S // O + 2):
        i = X * S // O + t
        w = np.maximum(np.minimum((X + 1) * S, (i + 1) * O) - np.maximum(X * S, i * O), 0)
        out += np.where(i < S, w, 0) * a[..., np.minimum(i, S - 1)]
    return out


def area(s, ow, oh):
    sh, sw = s.shape
    assert 255 * sw * sh + (sw * sh >> 1) < 2 ** 63           # (the definition's unsigned 64 bits hold it; so does int64 here)
    acc = _area_axis(_area_axis(np.asarray(s, np.int64), sw, ow).T, sh, oh).T
    return ((acc + (sw * sh >> 1)) // (sw * sh)).astype(np.uint8)


def area_dense(s, ow, oh):
    """The same through the weight matrices (small planes only)."""
    sh, sw = s.shape
    acc = area_weights(sh, oh) @ np.asarray(s, np.int64) @ area_weights(sw, ow).T
    return ((acc + (sw * sh >> 1)) // (sw * sh)).astype(np.uint8)


FILTERS = {"bilinear": bilinear, "area": area}


def normalise(c, scale, bias, dtype=np.float32):
    """uint8 -> float32: one rounded multiply, one rounded add; float16: that value converted, round to nearest even."""
    v = np.asarray(c).astype(np.float32) * np.float32(scale)
    v = v + np.float32(bias)
    assert v.dtype == np.float32
    return v if dtype == np.float32 else v.astype(np.float16)


def resize(planes, pixel_fmt, size, fmt="rgb_planar", filt="area", rect=None, dtype=np.uint8, scale=None, bias=None):
    """What thip_picture_resize writes: a list of three planes for "ycbcr", one (H, W, 3) / (H, W, 4) / (3, H, W) array
    otherwise; size = (out_width, out_height)."""
    src = source_planes(planes, pixel_fmt, rect)
    f = FILTERS[filt]
    Y, Cb, Cr = (f(s, ow, oh) for s, (ow, oh) in zip(src, output_sizes(fmt, size[0], size[1], pixel_fmt)))
    if fmt == "ycbcr":
        return [Y, Cb, Cr]
    R, G, B = picture_ref.ycbcr_to_rgb(Y, Cb, Cr)
    if fmt == "rgb":
        return np.stack([R, G, B], -1)
    if fmt == "rgba":
        return np.stack([R, G, B, np.full_like(R, 255)], -1)
    if fmt != "rgb_planar":
        raise ValueError(fmt)
    if dtype == np.uint8:
        return np.stack([R, G, B], 0)
    return np.stack([normalise(c, scale[k], bias[k], dtype) for k, c in enumerate((R, G, B))], 0)
