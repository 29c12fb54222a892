"""enc_rate_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s bitrate mode (include/theoraenc_hip.h, "Bitrate mode") in
numpy: the probe E[q] and the controller, to compare the library's choices with exactly.

The packets at a chosen qi are tests/enc_ref.py's (key frames) and tests/enc_inter_ref.py's (inter frames); the transform and the
quantiser are the oracle's.  The token counting here is a vectorised statement of enc_ref.block_tokens with every EOB its own token.
"""
import numpy as np

import oracle
from tests import enc_ref, enc_inter_ref
from tests.enc_ref import ZIGZAG
from tests.enc_inter_ref import INTRA, MV, NOMV

EXTRA_BITS = np.array([0, 0, 0, 2, 3, 4, 12, 3, 6, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 4, 5, 6, 10, 1, 1, 1, 1, 1, 3, 4, 2, 3], np.int64)
HG = np.array([enc_ref.huff_group(z) for z in range(65)], np.int64)   # (index 64: never used)
DROP_FRAMES, CAP_OVERFLOW, CAP_UNDERFLOW = 1, 2, 4


def code_lengths(setup):
    return np.array([[len(setup.codes[h].get(t, "")) for t in range(32)] for h in range(80)], np.int64)


def _value_token(a):
    """enc_ref's smallest value token of non-zero levels a (array)."""
    aa, s = np.abs(a), (a < 0).astype(np.int64)
    return np.select([aa == 1, aa == 2, aa <= 6, aa <= 8, aa <= 12, aa <= 20, aa <= 36, aa <= 68],
                     [9 + s, 11 + s, 10 + aa, 17, 18, 19, 20, 21], 22)


def token_hist(vals, chroma):
    """Tokens of blocks vals [N, 64] (zig-zag, DC the residual), each EOB its own token: counts [2][5][32] by (chroma, Huffman group
    of the start index, token) -- enc_ref.block_tokens, vectorised."""
    hist = np.zeros((2, 5, 32), np.int64)
    n = len(vals)
    if not n:
        return hist
    nz = vals != 0
    idx = np.arange(64)
    last = np.where(nz, idx, -1)
    prev = np.maximum.accumulate(np.concatenate([np.full((n, 1), -1), last[:, :-1]], 1), axis=1)   # last non-zero before z
    b, z = np.nonzero(nz)
    a, start = vals[b, z], prev[b, z] + 1
    gap = z - start
    cc = chroma[b].astype(np.int64)
    aa = np.abs(a)
    cat1 = (aa == 1) & (gap >= 1) & (gap <= 17)
    cat2 = ~cat1 & ((aa == 2) | (aa == 3)) & (gap >= 1) & (gap <= 3)
    plain = ~cat1 & ~cat2
    t1 = np.where(gap <= 5, 22 + gap, np.where(gap <= 9, 28, 29))
    t2 = np.where(gap == 1, 30, 31)
    np.add.at(hist, (cc[cat1], HG[start[cat1]], t1[cat1]), 1)
    np.add.at(hist, (cc[cat2], HG[start[cat2]], t2[cat2]), 1)
    zr = plain & (gap > 0)
    np.add.at(hist, (cc[zr], HG[start[zr]], np.where(gap[zr] <= 8, 7, 8)), 1)
    np.add.at(hist, (cc[plain], HG[z[plain]], _value_token(a[plain])), 1)
    end = last.max(1) + 1
    eob = end < 64
    np.add.at(hist, (chroma[eob].astype(np.int64), HG[end[eob]], 0), 1)
    return hist


def hist_bits(hist, lens):
    """The least bits of each table choice (DC luma, DC chroma, AC luma, AC chroma) plus the extra bits."""
    bits = int((hist.sum((0, 1)) * EXTRA_BITS).sum())
    for c in range(4):
        ac, cc = c >> 1, c & 1
        groups = range(1, 5) if ac else range(0, 1)
        bits += min(sum(int(hist[cc, hg] @ lens[16 * hg + t]) for hg in groups) for t in range(16))
    return bits


def _tdiv(a, b):
    return np.sign(a) * (np.abs(a) // b)


def dc_pred_masked(q, avail):
    """Spec 7.8 over one plane's quantised DCs q [nv, nh] (row 0 at the bottom) where a neighbour counts when avail(its index, mine)
    -- avail: [nv, nh, 4] booleans for (left, upper-left, upper, upper-right), already false outside the plane.  Mask 0 gives 0."""
    nv, nh = q.shape
    z = np.zeros_like(q)
    l = np.concatenate([z[:, :1], q[:, :-1]], 1)
    u = np.concatenate([z[:1], q[:-1]], 0)
    ul = np.concatenate([z[:, :1], u[:, :-1]], 1)
    ur = np.concatenate([u[:, 1:], z[:, :1]], 1)
    m = avail[..., 0] * 1 + avail[..., 1] * 2 + avail[..., 2] * 4 + avail[..., 3] * 8
    l, ul, u, ur = (np.where(avail[..., k], v, 0) for k, v in enumerate((l, ul, u, ur)))
    p15 = _tdiv(29 * (l + u) - 26 * ul, 32)
    p15 = np.where(np.abs(p15 - u) > 128, u, np.where(np.abs(p15 - l) > 128, l, np.where(np.abs(p15 - ul) > 128, ul, p15)))
    return np.select([np.isin(m, (1, 3)), m == 2, np.isin(m, (4, 6, 12)), m == 5, m == 8, np.isin(m, (9, 11, 13)), m == 10, m == 14,
                      np.isin(m, (7, 15))],
                     [l, ul, u, _tdiv(l + u, 2), ur, _tdiv(75 * l + 53 * ur, 128), _tdiv(ul + ur, 2), _tdiv(3 * (ul + ur) + 10 * u, 16),
                      p15], 0)


def _neighbour_avail(ok, same):
    """[nv, nh, 4] availability: the neighbour exists, ok (coded) and same(neighbour value, mine) for the class array `same`."""
    nv, nh = ok.shape
    out = np.zeros((nv, nh, 4), bool)
    for k, (dy, dx) in enumerate(((0, -1), (-1, -1), (-1, 0), (-1, 1))):
        ys, xs = np.mgrid[0:nv, 0:nh]
        yy, xx = ys + dy, xs + dx
        inside = (yy >= 0) & (xx >= 0) & (xx < nh)
        yc, xc = np.clip(yy, 0, nv - 1), np.clip(xx, 0, nh - 1)
        out[..., k] = inside & ok[yc, xc] & (same[yc, xc] == same)
    return out


class Probe:
    """E[q] of frames of one geometry (the probe of thip_rate.h, restated)."""

    def __init__(self, fw, fh, fmt, pic, setup):
        self.fw, self.fh, self.fmt, self.pic, self.setup = fw, fh, fmt, pic, setup
        self.geo = enc_inter_ref.Geometry(fw, fh, fmt)
        self.lens = code_lengths(setup)
        self.tabs = {(qti, p, q): setup.qmat(qti, p, q)[ZIGZAG].astype(np.uint16) for qti in range(2) for p in range(3)
                     for q in range(64)}

    def _src(self, planes):
        return [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]

    def _blocks(self, plane_rows, p):
        g = self.geo.planes[p]
        nh, nv = g["nhfrags"], g["nvfrags"]
        return plane_rows.reshape(nv, 8, nh, 8).transpose(0, 2, 1, 3).reshape(nv * nh, 64)

    def key(self, planes):
        src = self._src(planes)
        dct = [oracle.fdct8x8_batch((self._blocks(src[p], p) - 128).astype(np.int16)) for p in range(3)]
        E = np.zeros(64, np.int64)
        for q in range(64):
            hist = np.zeros((2, 5, 32), np.int64)
            for p, g in enumerate(self.geo.planes):
                lev = oracle.quantize_batch(dct[p], self.tabs[(0, p, q)])[0].astype(np.int64)
                vals = lev.copy()
                vals[:, 0] = enc_ref.dc_predict(lev[:, 0], g["nhfrags"], g["nvfrags"])
                hist += token_hist(vals, np.full(len(vals), p > 0))
            E[q] = 28 + hist_bits(hist, self.lens)
        return E

    def inter(self, planes, ref):
        """ref: the reference (three planes, bitstream row order, the decoder's PREV)."""
        geo = self.geo
        src = self._src(planes)
        mode0, mvx, mvy, s0, si, smv = search_stats(src[0], ref[0])
        res = {INTRA: [], NOMV: [], MV: []}   # per plane: coefficients [nfrags_p, 64] zig-zag
        for p, g in enumerate(geo.planes):
            nh = g["nhfrags"]
            fi = g["froffset"] + np.arange(g["nfrags"])
            mb = geo.mb_of[fi]
            fy, fx = (fi - g["froffset"]) // nh, (fi - g["froffset"]) % nh
            r = np.arange(8)
            Y = fy[:, None, None] * 8 + r[None, :, None]
            X = fx[:, None, None] * 8 + r[None, None, :]
            qx, qy = p > 0 and geo.hdec, p > 0 and geo.vdec
            pix = src[p][Y, X]
            zero = np.zeros(len(fi), np.int64)[:, None, None]
            for v, pred in ((INTRA, 128), (NOMV, enc_inter_ref.predict(ref[p], X, Y, zero, zero, qx, qy)),
                            (MV, enc_inter_ref.predict(ref[p], X, Y, mvx[mb][:, None, None], mvy[mb][:, None, None], qx, qy))):
                res[v].append(oracle.fdct8x8_batch((pix - pred).reshape(-1, 64).astype(np.int16)))
        nh0 = geo.planes[0]["nhfrags"]
        E = np.zeros(64, np.int64)
        for q in range(64):
            lam = int(self.tabs[(1, 0, q)][1])
            mode = np.where(smv + lam < s0, MV, NOMV)
            mode = np.where(si + 4 * lam < np.where(mode == MV, smv, s0), INTRA, mode)
            hist = np.zeros((2, 5, 32), np.int64)
            coded_all = np.zeros(geo.nfrags, bool)
            for p, g in enumerate(geo.planes):
                fi = g["froffset"] + np.arange(g["nfrags"])
                bm = mode[geo.mb_of[fi]]
                lev = np.zeros((len(fi), 64), np.int64)
                for v, qti in ((INTRA, 0), (NOMV, 1), (MV, 1)):
                    sel = bm == v
                    if sel.any():
                        lev[sel] = oracle.quantize_batch(res[v][p][sel], self.tabs[(qti, p, q)])[0]
                coded = (bm != NOMV) | (lev != 0).any(1)
                coded_all[fi] = coded
                nv, nh = g["nvfrags"], g["nhfrags"]
                cls = (bm != INTRA).reshape(nv, nh)
                avail = _neighbour_avail(coded.reshape(nv, nh), cls)
                dc = lev[:, 0].reshape(nv, nh)
                vals = lev[coded].copy()
                vals[:, 0] = (dc - dc_pred_masked(dc, avail)).reshape(-1)[coded]
                hist += token_hist(vals, np.full(len(vals), p > 0))
            # side bits: 3 a macro block with a coded luma block, 12 more when it is MV
            c0 = coded_all[:geo.planes[0]["nfrags"]].reshape(-1, nh0)
            mbc = (c0[0::2, 0::2] | c0[0::2, 1::2] | c0[1::2, 0::2] | c0[1::2, 1::2]).reshape(-1)
            side = 3 * int(mbc.sum()) + 12 * int((mbc & (mode == MV)).sum())
            E[q] = 25 + geo.nfrags // 8 + side + hist_bits(hist, self.lens)
        return E


def search_stats(src, ref):
    """enc_inter_ref.motion_search's statistics before the mode decision: (None, mvx, mvy, S0, SI, Smv), the half-pel vector of
    every macro block whatever its mode."""
    # (motion_search with the decision left out: it zeroes the vector of a macro block that is not MV)
    H, W = src.shape
    nmy, nmx = H // 16, W // 16
    s = src.astype(np.int64)
    pad = np.pad(ref, 16, mode="edge").astype(np.int64)
    keys = np.empty((31 * 31, nmy * nmx), np.int64)
    for ci in range(31 * 31):
        dy, dx = ci // 31 - 15, ci % 31 - 15
        d = np.abs(s - pad[16 + dy:16 + dy + H, 16 + dx:16 + dx + W]).reshape(nmy, 16, nmx, 16).sum((1, 3)).reshape(-1)
        keys[ci] = (d << 32) | ((2 * (abs(dx) + abs(dy))) << 16) | ci
    best = keys.min(0)
    s0 = keys[15 * 31 + 15] >> 32
    bci = best & 0xFFFF
    bdx, bdy = bci % 31 - 15, bci // 31 - 15
    y0 = (np.arange(nmy * nmx) // nmx) * 16
    x0 = (np.arange(nmy * nmx) % nmx) * 16
    r = np.arange(16)
    Y = y0[:, None, None] + r[None, :, None]
    X = x0[:, None, None] + r[None, None, :]
    sblk = s[Y, X]
    cur = (best >> 16 << 16) | 4
    for k9 in (0, 1, 2, 3, 5, 6, 7, 8):
        mvx, mvy = 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1
        p = enc_inter_ref.predict(ref, X, Y, mvx[:, None, None], mvy[:, None, None], False, False)
        sad = np.abs(sblk - p).sum((1, 2))
        cur = np.minimum(cur, (sad << 32) | ((np.abs(mvx) + np.abs(mvy)) << 16) | k9)
    k9 = cur & 0xFFFF
    mvx, mvy = 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1
    b4 = sblk.reshape(-1, 2, 8, 2, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 4, 64)
    mean = (b4.sum(2) + 32) >> 6
    si = np.abs(b4 - mean[:, :, None]).sum((1, 2))
    return None, mvx, mvy, s0, si, cur >> 32


class Controller:
    """The controller of theoraenc_hip.h, step for step (Python integers)."""

    def __init__(self, bitrate, fps, inter, kf_interval, shift, flags=DROP_FRAMES | CAP_OVERFLOW, buffer=None):
        self.bitrate, self.fps, self.inter, self.K, self.shift = bitrate, fps, inter, kf_interval, shift
        self.flags, self.buffer = flags, buffer
        self.started = False
        self.c = [65536, 65536]
        self.L = [None, None]

    def _targets(self):
        self.T = min(max(self.bitrate * self.fps[1] // self.fps[0], 32), 1 << 40)
        self.R = self.T * self.D
        self.Fstar = self.R // 2

    def _caps(self):
        if self.flags & CAP_OVERFLOW:
            self.F = min(self.F, self.R)
        if self.flags & CAP_UNDERFLOW:
            self.F = max(self.F, 0)

    def set_bitrate(self, b):
        self.bitrate = b
        if self.started:
            self._targets()
            self.F = min(self.F, self.R)

    def set_buffer(self, d):
        """TH_ENCCTL_SET_RATE_BUFFER: D clamped to [12, 256]; mid-stream R and F* follow and F = min(F, R)."""
        self.buffer = min(max(d, 12), 256)
        if self.started:
            self.D = self.buffer
            self._targets()
            self.F = min(self.F, self.R)
        return self.buffer

    def choose(self, E, key, f, keypos, first, lastkey, dups):
        """-> (qi or -1 to drop, record)."""
        if not self.started:
            self.D = self.buffer or min(max(self.K if self.inter else 1, 12), 256)
            self._targets()
            self.F = self.Fstar
            self.started = True
        t = 0 if key else 1
        E = [int(x) for x in E]
        self.L[t] = E
        nk = sum(1 for m in range(f + 1, f + self.D) if not self.inter or (m - keypos) % self.K == 0)
        ni = self.D - 1 - nk
        cur, fut = [], []
        for q in range(64):
            cur.append(E[q] * self.c[t] >> 16)
            kt = self.L[0][q] * self.c[0] >> 16 if self.L[0] else None
            it = self.L[1][q] * self.c[1] >> 16 if self.L[1] else None
            if it is None:
                it = kt // 4
            if kt is None:
                kt = 4 * it
            fut.append(nk * kt + ni * it)
        S = self.F + self.D * self.T - self.Fstar
        qi = max([q for q in range(64) if cur[q] + fut[q] <= S], default=0)
        drop = bool(self.flags & DROP_FRAMES) and not first and self.F + self.T - cur[0] < 0 and lastkey >= 0 and \
            f - lastkey + dups < (1 << self.shift)
        rec = dict(fullness_before=self.F, spend=S, estimate=cur[qi], target=self.T, dropped=int(drop))
        if drop:
            self.F += self.T
            self._caps()
            rec.update(fullness_after=self.F, corr=list(self.c))
            return -1, rec
        self.E = E
        return qi, rec

    def coded(self, key, qi, A):
        t = 0 if key else 1
        self.F += self.T - A
        self._caps()
        self.c[t] = min(max((self.c[t] + (A << 16) // max(self.E[qi], 1)) // 2, 4096), 1 << 20)
        return dict(fullness_after=self.F, corr=list(self.c), actual=A)

    def dup(self):
        if not self.started:
            return None
        before = self.F
        self.F += self.T
        self._caps()
        return dict(fullness_before=before, fullness_after=self.F)


class RateStream:
    """The stream th_encode_* makes in bitrate mode: frame(planes, dups) -> list of (packet, record) (the frame's, then its
    duplicates')."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, fps=(30, 1), inter=False, kf_interval=64, shift=6, flags=DROP_FRAMES |
                 CAP_OVERFLOW, buffer=None):
        self.enc = enc_inter_ref.InterEncoder(fw, fh, fmt, pic, setup, kf_interval if inter else 1, shift)
        self.probe = Probe(fw, fh, fmt, pic, setup)
        self.ctl = Controller(bitrate, fps, inter, kf_interval, shift, flags, buffer)
        self.inter, self.K, self.shift = inter, kf_interval, shift
        self.cur, self.key, self.qi = -1, -1, 0

    def close(self):
        self.enc.close()

    def frame(self, planes, dups=0):
        f = self.cur + 1
        off = f - self.key
        key = not self.inter or self.key < 0 or off >= self.K or off + dups >= (1 << self.shift)
        if key:
            E = self.probe.key(planes)
        else:
            E = self.probe.inter(planes, [self.enc.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)])
        qi, rec = self.ctl.choose(E, key, f, f if key else self.key, self.cur < 0, self.key, dups)
        rec.update(probe=list(E), key=int(key and qi >= 0))
        out = []
        if qi < 0:
            rec.update(qi=self.qi)
            out.append((b"", rec))
        else:
            # the restated encoders decide key / inter by their own counters: keep them in step with the drops
            self.enc.cur, self.enc.key = self.cur, self.key
            r = self.enc.frame(planes, qi, dups=dups)
            assert r["key"] == key
            if key:
                self.key = f
            self.qi = qi
            rec.update(qi=qi)
            rec.update(self.ctl.coded(key, qi, 8 * len(r["packet"])))
            out.append((r["packet"], rec))
        self.cur = f
        for _ in range(dups):
            self.cur += 1
            d = self.ctl.dup()
            out.append((b"", dict(d, qi=self.qi, duplicate=1)))
        return out
