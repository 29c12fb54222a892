"""numpy restatement of thip_picture_compare's definition (include/theora_hip.h), written from the header's text: the source
rectangles, the squared differences per plane and per 8x8 block, and the integer SSIM.  int64 throughout; numpy's // floors, C's /
rounds toward zero, so the division is made from magnitudes and the sign put back.  Planes are in DISPLAY order (row 0 at the top),
the full coded frame, as ycbcr_out() gives them."""
import numpy as np

from tests.picture_resize_ref import decs, source_planes  # noqa: F401  (the rectangles are thip_picture_resize's)

SSE, SSIM = 1, 2
C1, C2 = 26634, 239708      # floor(64^2 (0.01 * 255)^2), floor(64^2 (0.03 * 255)^2)


def cdiv(n, d):
    """C's n / d on int64 arrays: rounded toward zero."""
    n, d = np.asarray(n, np.int64), np.asarray(d, np.int64)
    q = np.abs(n) // np.abs(d)
    return np.where((n < 0) != (d < 0), -q, q)


def window_terms(sx, sy, sxx, syy, sxy):
    """a, b, c, d, q1, q2, w of windows given their five sums (int64 arrays)."""
    sx, sy, sxx, syy, sxy = (np.asarray(v, np.int64) for v in (sx, sy, sxx, syy, sxy))
    a = 2 * sx * sy + C1
    b = sx * sx + sy * sy + C1
    c = 2 * (64 * sxy - sx * sy) + C2
    d = (64 * sxx - sx * sx) + (64 * syy - sy * sy) + C2
    q1 = cdiv(a << 20, b)
    q2 = cdiv(c * (1 << 20), d)      # (c may be negative: a product, not a shift, as in C where c << 20 of a negative c is not defined)
    w = cdiv(q1 * q2, 1 << 20)
    return a, b, c, d, q1, q2, w


def _box(m, size, step):
    """Sums of m over every size x size box at multiples of `step` that lies wholly inside, through an integral image (exact: int64)."""
    h, w = m.shape
    ny, nx = ((h - size) // step + 1 if h >= size else 0), ((w - size) // step + 1 if w >= size else 0)
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = m.cumsum(0).cumsum(1)
    y, x = np.arange(ny) * step, np.arange(nx) * step
    return ii[np.ix_(y + size, x + size)] - ii[np.ix_(y, x + size)] - ii[np.ix_(y + size, x)] + ii[np.ix_(y, x)]


def window_sums(s, r):
    """The five sums sx, sy, sxx, syy, sxy of every 8x8 window at step 4 that lies wholly inside the plane: arrays of shape (windows
    down, windows across), empty where the plane is narrower or shorter than 8."""
    s, r = np.asarray(s, np.int64), np.asarray(r, np.int64)
    return [_box(m, 8, 4) for m in (s, r, s * s, r * r, s * r)]


def window_q20(s, r):
    """w of every window of the plane pair."""
    return window_terms(*window_sums(s, r))[6]


def block_sse(s, r):
    """(s - r)^2 summed over the 8x8 blocks counted from the top-left; edge blocks hold what is inside the plane."""
    d = np.asarray(s, np.int64) - np.asarray(r, np.int64)
    h, w = d.shape
    pad = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), np.int64)
    pad[:h, :w] = d * d
    return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8).sum((1, 3))


def compare_planes(src, ref, flags=SSE):
    """thip_picture_metrics as 12 Python ints (sse, samples, ssim_q20, windows by plane) for three plane pairs of equal shapes."""
    sse, samples, q20, win = [0] * 3, [0] * 3, [0] * 3, [0] * 3
    for p in range(3):
        s, r = np.asarray(src[p], np.int64), np.asarray(ref[p], np.int64)
        assert s.shape == r.shape
        if flags & SSE:
            sse[p] = int(((s - r) ** 2).sum())
            samples[p] = int(s.size)
        if flags & SSIM:
            w = window_q20(s, r)
            q20[p] = int(w.sum())
            win[p] = int(w.size)
    return sse + samples + q20 + win


def compare(planes, pixel_fmt, ref, flags=SSE, rect=None):
    """The record of a request: the rectangle `rect` (None: the whole frame) of the frame `planes` against the planes `ref`."""
    return compare_planes(source_planes(planes, pixel_fmt, rect), ref, flags)


def blocks(planes, pixel_fmt, ref, rect=None):
    return [block_sse(s, r) for s, r in zip(source_planes(planes, pixel_fmt, rect), ref)]


def ssim_float(s, r):
    """The usual real-valued SSIM of one 8x8 window: population moments, K1 = 0.01, K2 = 0.03, L = 255 (float64)."""
    s, r = np.asarray(s, np.float64).ravel(), np.asarray(r, np.float64).ravel()
    mx, my = s.mean(), r.mean()
    vx, vy = (s * s).mean() - mx * mx, (r * r).mean() - my * my
    cov = (s * r).mean() - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return (2 * mx * my + c1) * (2 * cov + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def psnr(sse, samples):
    """dump_psnr's 10 (log10(255^2) + log10(samples) - log10(sse))."""
    import math
    return 10 * (math.log10(255 * 255) + math.log10(samples) - math.log10(sse))
