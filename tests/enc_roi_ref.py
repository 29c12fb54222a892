"""enc_roi_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s region-of-interest maps (TH_ENCCTL_THIP_SET_ROI_MAP;
include/theoraenc_hip.h, "Region of interest") in numpy, to compare the library's scales and packets with.  Integer arithmetic
throughout; every division rounds down and every >> is arithmetic (numpy's and Python's are).

roi_scales is the rule; RoiEncoder is tests/enc_rdq_ref.RdqEncoder (and through it the skip decision, the rate-distortion mode
decision, masking and block qi) with the rule's scales where those restatements take masking's.  They fetch them through
tests/enc_mask_ref.scales at three places, and only when `k and delta`: RoiEncoder swaps that source for the duration of a frame.
"""
import numpy as np

from tests import enc_mask_ref as K
from tests import enc_rdq_ref as Q

ONE = 2048
T = [2048, 2139, 2233, 2332, 2435, 2543, 2656, 2774, 2896, 3025, 3158, 3298, 3444, 3597, 3756, 3922]   # round(2048 2^(f / 16))
SCALE_MIN, SCALE_MAX = 128, 32768


def roi_scale(e):
    """r of the exponent e (an int or an array), Q11."""
    e = np.asarray(e, np.int64)
    n = -e
    o, f = n >> 4, n & 15
    t = np.asarray(T, np.int64)[f]
    up = t << np.maximum(o, 0)
    sh = np.maximum(-o, 1)
    down = (t + (1 << (sh - 1))) >> sh
    return np.where(o >= 0, up, down)


def cells(coord, size, n):
    """The map cell of every luma coordinate (picture coordinates): clamp into the picture, then coord n / size."""
    return np.clip(np.asarray(coord, np.int64), 0, size - 1) * n // size


def exponents(geo, pic, fmt, map):
    """Every fragment's exponent e, [nfrags] in fragment raster order (rows from the bottom).  pic = (x, y, width, height) with y
    from the top; map [Hm][Wm], row 0 the picture's top row."""
    v = np.asarray(map, np.int64)
    hm, wm = v.shape
    px, py, pw, ph = pic
    out = np.empty(geo.nfrags, np.int64)
    for p, g in enumerate(geo.planes):
        hd, vd = (geo.hdec, geo.vdec) if p else (0, 0)
        nh, nv = g["nhfrags"], g["nvfrags"]
        cx = cells((np.arange(nh * 8) << hd) - px, pw, wm)      # by plane column
        cy = cells((np.arange(nv * 8) << vd) - py, ph, hm)      # by plane row, from the top
        full = v[cy[:, None], cx[None, :]]                      # the map at every sample of the plane
        S = full.reshape(nv, 8, nh, 8).sum((1, 3))              # by fragment row from the top, column
        out[g["froffset"]:g["froffset"] + g["nfrags"]] = ((np.flipud(S) + 32) >> 6).reshape(-1)
    return out


def roi_scales(geo, pic, fmt, map, mask_iscale=None):
    """(iscale [nfrags], stats) of the map: the final scale of every fragment, on top of masking's scales mask_iscale [nfrags] where
    given, and thip_enc_roi_stats' fields of the frame (exp_min, exp_max, exp_sum over the luma fragments; scale_min, scale_max over
    all)."""
    e = exponents(geo, pic, fmt, map)
    m = np.full(geo.nfrags, ONE, np.int64) if mask_iscale is None else np.asarray(mask_iscale, np.int64)
    i = np.clip((m * roi_scale(e) + 1024) >> 11, SCALE_MIN, SCALE_MAX)
    el = e[:geo.planes[0]["nfrags"]]
    return i, dict(exp_min=int(el.min()), exp_max=int(el.max()), exp_sum=int(el.sum()), scale_min=int(i.min()), scale_max=int(i.max()))


def from_octaves(x):
    """Encoder.set_roi's reading of a float map in octaves: clamp(round(16 x), -64, 64)."""
    return np.clip(np.rint(16.0 * np.asarray(x, np.float64)), -64, 64).astype(np.int8)


def rect_map(pic, rect, v):
    """examples/encoder_example_hip.c's --roi x,y,w,h,v: a map at macro-block resolution (16 picture pixels a cell), v where the
    cell's top-left picture pixel lies inside the rectangle (picture coordinates, y from the top), 0 elsewhere."""
    pw, ph = pic[2], pic[3]
    wm, hm = (pw + 15) // 16, (ph + 15) // 16
    x, y, w, h = rect
    m = np.zeros((hm, wm), np.int8)
    for cy in range(hm):
        for cx in range(wm):
            if x <= cx * 16 < x + w and y <= cy * 16 < y + h:
                m[cy, cx] = v
    return m


_SELF = object()
STAT_ZERO = dict(measured=0, exp_min=0, exp_max=0, exp_sum=0, scale_min=0, scale_max=0, clamped=0)


class RoiEncoder(Q.RdqEncoder):
    """The stream th_encode_* makes with a map set by TH_ENCCTL_THIP_SET_ROI_MAP: frame(planes, qi, dups, roi) takes the map in force
    for that frame (None: none; not given: self.roi, for the callers that know nothing of maps, tests/enc_rate_ref.RateStream among
    them).  It returns RdqEncoder's dict plus roi (TH_ENCCTL_THIP_GET_ROI_STATS as Encoder.roi_stats returns
    it, without roi_ms) and, for a frame that used the map, roi_iscale (the scales)."""

    roi = None

    def frame(self, planes, qi, dups=0, roi=_SELF):
        if roi is _SELF:
            roi = self.roi
        dims = dict(active=int(roi is not None), map_width=0 if roi is None else int(np.shape(roi)[1]),
                    map_height=0 if roi is None else int(np.shape(roi)[0]))
        if roi is None or not self.delta:
            out = super().frame(planes, qi, dups)
            out["roi"] = dict(dims, **STAT_ZERO)
            return out
        k, scales, activity = self.k, K.scales, K.activity
        used = {}

        def roi_source(act, kk, geo):
            m, A, amax = scales(act, k, geo) if k else (None, 0, 0)
            used["iscale"], used["stats"] = roi_scales(geo, self.pic, self.fmt, roi, m)
            return used["iscale"], A, amax

        K.scales = roi_source
        K.activity = activity if k else (lambda *a: None)
        self.k = k or 1   # (the three places ask `k and delta` first)
        try:
            out = super().frame(planes, qi, dups)
        finally:
            K.scales, K.activity, self.k = scales, activity, k
        if not k:
            out["mask"] = dict(ratio=0, measured=0, activity_avg=0, activity_max=0)
        if out["packet"] and used:
            out["roi"] = dict(dims, measured=1, clamped=0, **used["stats"])
            out["roi_iscale"] = used["iscale"]
        else:
            out["roi"] = dict(dims, **STAT_ZERO)
        return out
