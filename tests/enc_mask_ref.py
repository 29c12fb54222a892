"""enc_mask_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s activity masking (TH_ENCCTL_THIP_SET_MASKING;
include/theoraenc_hip.h, "Activity masking") in numpy, to compare the library's packets with byte for byte.  Integer arithmetic
throughout (Python ints where a product may pass 64 bits in a test's grid).

The activity is the oracle's oc_mb_activity over the frame the encoder transforms (tests/enc_ref.frame_planes: the picture, clamped
outward); the stream is tests/enc_bqi_ref.BqiEncoder's with one change, the block's lambda in the choice.
"""
import numpy as np

import oracle
from tests import enc_bqi_ref as B
from tests import enc_ref
from tests.enc_ref import ZIGZAG

ONE = 2048        # the scale's unit (Q11)
FLOOR = 64        # the least frame average
# a luma block's place in oracle.mb_cost_maps: position on the super block's Hilbert curve by (row & 3, column & 3); the macro block
# is super block << 2 | h >> 2, the entry h & 3
HILBERT = np.array([[0, 1, 14, 15], [3, 2, 13, 12], [4, 7, 8, 11], [5, 6, 9, 10]])


def luma_raster(maps, fw, fh):
    """An [nmbs, 4] map of oracle.mb_cost_maps (planes in bitstream row order) as [nv, nh]: by luma fragment row and column."""
    nh, nv = fw >> 3, fh >> 3
    nsbw = (nh + 3) >> 2
    by, bx = np.mgrid[0:nv, 0:nh]
    h = HILBERT[by & 3, bx & 3]
    mbi = (((by >> 2) * nsbw + (bx >> 2)) << 2) | (h >> 2)
    return np.asarray(maps)[mbi, h & 3]


def activity(planes, fw, fh, fmt, pic):
    """Every luma fragment's activity, [nluma] in fragment raster order, rows from the bottom as everywhere in the bitstream:
    oracle.mb_cost_maps over the frame planes (the picture region clamped outward)."""
    fp = [np.flipud(a) for a in enc_ref.frame_planes(planes, fw, fh, fmt, pic)]
    return luma_raster(oracle.mb_cost_maps(fp, fw, fh, fmt)[2], fw, fh).reshape(-1).astype(np.int64)


def average(act):
    """A = max(64, (sum a + n / 2) / n)."""
    n = len(act)
    return max(FLOOR, (int(np.asarray(act, np.int64).sum()) + n // 2) // n)


def luma_scale(a, A, k):
    """i = (2048 (k a + A) + (a + k A) / 2) / (a + k A), on Python ints."""
    a, A, k = int(a), int(A), int(k)
    den = a + k * A
    return (ONE * (k * a + A) + den // 2) // den


def chroma_scale(four):
    """Of a macro block's four luma scales: the least when none lies under 2048, else the second least; never under 2048."""
    i = sorted(int(v) for v in four)
    return max(i[0] if i[0] >= ONE else i[1], ONE)


def scales(act, k, geo):
    """(iscale [nfrags] in fragment raster order, A, the largest activity) of the activities act [nluma]."""
    act = np.asarray(act, np.int64)
    A = average(act)
    den = act + k * A
    luma = (ONE * (k * act + A) + den // 2) // den     # (a < 2^32 and k <= 16: no term passes 2^48)
    nh = geo.planes[0]["nhfrags"]
    out = np.empty(geo.nfrags, np.int64)
    nl = geo.planes[0]["nfrags"]
    out[:nl] = luma
    lum2 = luma.reshape(-1, nh)
    for fi in range(nl, geo.nfrags):
        mb = int(geo.mb_of[fi])
        y, x = 2 * (mb // geo.nmbx), 2 * (mb % geo.nmbx)
        out[fi] = chroma_scale(lum2[y:y + 2, x:x + 2].reshape(-1))
    return out, A, int(act.max())


def choose(dct, tabs, bits, iscale, bias=B.FLAG_BIAS):
    """enc_bqi_ref.choose with lambda_b = (lambda iscale_b + 1024) >> 11 a block: iscale [n]."""
    levs, dist = [], []
    c = dct.astype(np.int64)
    for tab in tabs:
        q, _ = oracle.quantize_batch(dct, np.asarray(tab, np.uint16))
        q = q.astype(np.int64)
        levs.append(q)
        e = c[:, 1:] - q[:, 1:] * np.asarray(tab, np.int64)[1:]
        dist.append((e * e).sum(1))
    s = int(tabs[0][1])
    lam = (s * s * B.LAM_NUM) >> B.LAM_SHIFT
    n = dct.shape[0]
    qii = np.zeros(n, np.int64)
    out = levs[0].copy()
    for i in range(n):
        lb = (lam * int(iscale[i]) + 1024) >> 11
        best = None
        for k in range(len(tabs)):
            j = int(dist[k][i]) + lb * (B.ac_bits(levs[k][i], bits) + (bias if k else 0))
            if best is None or j < best:
                best, qii[i] = j, k
        if qii[i]:
            out[i, 1:] = levs[qii[i]][i, 1:]
    return out, qii


class MaskEncoder(B.BqiEncoder):
    """The stream th_encode_* makes with TH_ENCCTL_THIP_SET_BLOCK_QI = delta and TH_ENCCTL_THIP_SET_MASKING = k.  frame() returns
    BqiEncoder's dict plus mask (TH_ENCCTL_THIP_GET_MASK_STATS as Encoder.mask_stats returns it, without mask_ms)."""

    def __init__(self, fw, fh, fmt, pic, setup, kf_interval, shift, delta, k, modes=False, bias=B.FLAG_BIAS):
        super().__init__(fw, fh, fmt, pic, setup, kf_interval, shift, delta, modes, bias)
        self.k = k
        self._mask = None

    def frame(self, planes, qi, dups=0):
        self._planes = planes
        self._mask = None
        out = super().frame(planes, qi, dups)
        m = self._mask if out["packet"] else None
        out["mask"] = dict(ratio=self.k, measured=int(m is not None), activity_avg=m[0] if m else 0, activity_max=m[1] if m else 0)
        return out

    def _code(self, src, pred, intra, qis, key):
        """BqiEncoder._code with the block's scale in the choice; without block qi (delta 0) or masking (k 0) it is BqiEncoder's."""
        if not self.k or not self.delta:
            return super()._code(src, pred, intra, qis, key)
        geo, setup = self.geo, self.setup
        iscale, A, amax = scales(activity(self._planes, self.fw, self.fh, self.fmt, self.pic), self.k, geo)
        self._mask = (A, amax)
        lev = np.zeros((geo.nfrags, 64), np.int64)
        qii = np.zeros(geo.nfrags, np.int64)
        qti_of = np.where(intra, 0, 1)
        ht = self.hti[key]
        for p, g in enumerate(geo.planes):
            nh = g["nhfrags"]
            fi = g["froffset"] + np.arange(g["nfrags"])
            fy, fx = (fi - g["froffset"]) // nh, (fi - g["froffset"]) % nh
            r = np.arange(8)
            Y = fy[:, None, None] * 8 + r[None, :, None]
            X = fx[:, None, None] * 8 + r[None, None, :]
            res = (src[p][Y, X] - pred[p]).reshape(-1, 64)
            dct = oracle.fdct8x8_batch(res.astype(np.int16))
            bits = B.token_bits(setup, ht[int(p > 0)])
            for t in range(2):
                sel = qti_of[fi] == t
                if sel.any():
                    tabs = [setup.qmat(t, p, q)[ZIGZAG] for q in qis]
                    lev[fi[sel]], qii[fi[sel]] = choose(dct[sel], tabs, bits, iscale[fi[sel]], self.bias)
        return lev, qii, qti_of
