"""numpy restatement of thip_picture_in's definition (include/theora_hip.h): the integer R'G'B' -> Y'CbCr matrix, and chroma as the
mean over the 1 << (hdec + vdec) pixels a sample of the spec 4.4 chroma region covers, positions outside the picture taking the
nearest picture pixel.  Pictures are in display order (row 0 at the top)."""
import numpy as np


def luma(R, G, B):
    R, G, B = (np.asarray(c, np.int32) for c in (R, G, B))
    return 16 + ((16829 * R + 33039 * G + 6416 * B + 32768) >> 16)


def chroma(SR, SG, SB, s):
    """(Cb, Cr) of the sums over 1 << s pixels: one rounding, after the mean."""
    SR, SG, SB = (np.asarray(c, np.int32) for c in (SR, SG, SB))
    half, sh = 1 << (15 + s), 16 + s
    return (128 + ((-9714 * SR - 19070 * SG + 28784 * SB + half) >> sh),
            128 + ((28784 * SR - 24103 * SG - 4681 * SB + half) >> sh))


def spec_ycbcr(R, G, B, kr=0.299, kb=0.114):
    """The specification's real-valued conversion (offsets 16 / 128, excursions 219 / 224), not rounded; R, G, B may be means."""
    r, g, b = (np.asarray(c, np.float64) / 255 for c in (R, G, B))
    y = kr * r + (1 - kr - kb) * g + kb * b
    return 16 + 219 * y, 128 + 224 * (b - y) / (2 * (1 - kb)), 128 + 224 * (r - y) / (2 * (1 - kr))


def decimation(pixel_fmt):
    return int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))


def plane_shapes(width, height, pixel_fmt, pic_x=0, pic_y=0):
    hdec, vdec = decimation(pixel_fmt)
    cw = ((pic_x + width + hdec) >> hdec) - (pic_x >> hdec)
    ch = ((pic_y + height + vdec) >> vdec) - (pic_y >> vdec)
    return [(height, width), (ch, cw), (ch, cw)]


def split(image, fmt):
    """R, G, B planes of an image in one of the three formats."""
    image = np.asarray(image)
    if fmt in ("rgb", "rgba"):
        assert image.ndim == 3 and image.shape[2] == (3 if fmt == "rgb" else 4)
        return image[..., 0], image[..., 1], image[..., 2]
    if fmt == "rgb_planar":
        return image[0], image[1], image[2]
    raise ValueError(fmt)


def picture_in(image, pixel_fmt, fmt="rgb", pic_x=0, pic_y=0):
    """What thip_picture_in writes: [Y, Cb, Cr] as uint8 planes of plane_shapes' shapes."""
    R, G, B = (np.asarray(c, np.int32) for c in split(image, fmt))
    h, w = R.shape
    hdec, vdec = decimation(pixel_fmt)
    (_, _), (ch, cw) = plane_shapes(w, h, pixel_fmt, pic_x, pic_y)[:2]
    cx0, cy0 = pic_x >> hdec, pic_y >> vdec
    SR, SG, SB = (np.zeros((ch, cw), np.int32) for _ in range(3))
    for dy in range(1 + vdec):
        ys = np.clip(((cy0 + np.arange(ch)) << vdec) + dy - pic_y, 0, h - 1)
        for dx in range(1 + hdec):
            xs = np.clip(((cx0 + np.arange(cw)) << hdec) + dx - pic_x, 0, w - 1)
            SR += R[ys][:, xs]
            SG += G[ys][:, xs]
            SB += B[ys][:, xs]
    Cb, Cr = chroma(SR, SG, SB, hdec + vdec)
    return [p.astype(np.uint8) for p in (luma(R, G, B), Cb, Cr)]
