"""numpy restatement of thip_picture_out's definitions (include/theora_hip.h): the crop, the integer Y'CbCr -> R'G'B' matrix and
the two chroma upsampling rules.  Planes are in DISPLAY order (row 0 at the top), the full coded frame, as ycbcr_out() gives them."""
import numpy as np


def ycbcr_to_rgb(Y, Cb, Cr):
    """The library's exact integer form."""
    y = np.asarray(Y, np.int64) - 16
    u = np.asarray(Cb, np.int64) - 128
    v = np.asarray(Cr, np.int64) - 128
    R = (76309 * y + 104597 * v + 32768) >> 16
    G = (76309 * y - 25675 * u - 53279 * v + 32768) >> 16
    B = (76309 * y + 132201 * u + 32768) >> 16
    return [np.clip(c, 0, 255).astype(np.uint8) for c in (R, G, B)]


def spec_rgb(Y, Cb, Cr, kr=0.299, kb=0.114):
    """The specification's real-valued conversion (offsets 16 / 128, excursions 219 / 224), rounded to 8 bits."""
    y = (np.asarray(Y, np.float64) - 16) / 219
    pb = (np.asarray(Cb, np.float64) - 128) / 224
    pr = (np.asarray(Cr, np.float64) - 128) / 224
    R = y + 2 * (1 - kr) * pr
    G = y - 2 * (1 - kb) * kb / (1 - kb - kr) * pb - 2 * (1 - kr) * kr / (1 - kb - kr) * pr
    B = y + 2 * (1 - kb) * pb
    return [np.round(255 * np.clip(c, 0, 1)).astype(np.int64) for c in (R, G, B)]


def _axis(n_full, dec):
    """Per full-resolution index: the sample's own chroma index and its neighbour's (centred siting), clamped to the plane."""
    i = np.arange(n_full)
    k = i >> dec
    nb = np.where(i & 1, k + 1, k - 1) if dec else k
    return k, np.clip(nb, 0, ((n_full + dec) >> dec) - 1)


def upsample(c, width, height, hdec, vdec, mode):
    """A chroma plane brought to width x height: mode "nearest" or "linear"."""
    c = np.asarray(c, np.int64)
    kx, nx = _axis(width, hdec)
    ky, ny = _axis(height, vdec)
    a = c[ky][:, kx]
    if mode == "nearest" or not (hdec or vdec):
        return a.astype(np.uint8)
    if hdec and vdec:
        b, cc, d = c[ky][:, nx], c[ny][:, kx], c[ny][:, nx]
        return ((9 * a + 3 * b + 3 * cc + d + 8) >> 4).astype(np.uint8)
    b = c[ky][:, nx] if hdec else c[ny][:, kx]
    return ((3 * a + b + 2) >> 2).astype(np.uint8)


def picture(planes, pixel_fmt, fmt, chroma="linear", rect=None):
    """What thip_picture_out writes for the display-order planes `planes`: a list of three planes for "ycbcr", one
    (H, W, 3) / (H, W, 4) / (3, H, W) array otherwise."""
    hdec, vdec = int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))
    H, W = planes[0].shape
    x, y, w, h = rect if rect is not None else (0, 0, W, H)
    if fmt == "ycbcr":
        out = [planes[0][y:y + h, x:x + w]]
        for p in (1, 2):
            out.append(planes[p][y >> vdec:(y + h + vdec) >> vdec, x >> hdec:(x + w + hdec) >> hdec])
        return out
    cb = upsample(planes[1], W, H, hdec, vdec, chroma)
    cr = upsample(planes[2], W, H, hdec, vdec, chroma)
    R, G, B = (c[y:y + h, x:x + w] for c in ycbcr_to_rgb(planes[0], cb, cr))
    if fmt == "rgb":
        return np.stack([R, G, B], -1)
    if fmt == "rgba":
        return np.stack([R, G, B, np.full_like(R, 255)], -1)
    if fmt == "rgb_planar":
        return np.stack([R, G, B], 0)
    raise ValueError(fmt)
