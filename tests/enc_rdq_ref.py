"""enc_rdq_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s level choice (TH_ENCCTL_THIP_SET_RD_QUANT;
include/theoraenc_hip.h, "Level choice") in plain loops over Python ints, to compare the library's levels and packets with byte for
byte.

What is new here: the token cost of one value after a run (value_tokens: the header's token rule, which enc_ref.block_tokens states
for whole blocks), the backward programme (choose_block), and the same minimum by brute force over all 2^n choices in lexicographic
order (brute_block).  Everything else is the restated encoders': RdqEncoder is enc_skip_ref.SkipEncoder with the choice between the
block coding and the token writer; with w = 0 it is SkipEncoder.
"""
import itertools

import numpy as np

import oracle
from tests import enc_bqi_ref as B
from tests import enc_inter_ref as IR
from tests import enc_mask_ref as K
from tests import enc_ref
from tests import enc_skip_ref as S
from tests.enc_ref import ZIGZAG
from tests.packref import EXTRA_BITS


def group(zs):
    """The AC Huffman group (0..3) of a token that starts at zig-zag index zs >= 1."""
    return 0 if zs <= 5 else 1 if zs <= 14 else 2 if zs <= 27 else 3


def value_token(v):
    """The smallest value token of v != 0 (spec Table 7.38)."""
    a = abs(v)
    for tok, hi in ((9, 1), (11, 2)):
        if a == hi:
            return tok + (v < 0)
    if a <= 6:
        return 10 + a
    for tok, hi in ((17, 8), (18, 12), (19, 20), (20, 36), (21, 68)):
        if a <= hi:
            return tok
    return 22


def value_tokens(v, z, nxt):
    """[(token, start index)] of the value v != 0 at zig-zag index z when the block's previous token ended before index nxt: a combined
    run-and-value token where one fits, else a zero run (when z > nxt) and the smallest value token."""
    gap, a = z - nxt, abs(v)
    if a == 1 and 1 <= gap <= 17:
        return [(22 + gap if gap <= 5 else 28 if gap <= 9 else 29, nxt)]
    if a in (2, 3) and 1 <= gap <= 3:
        return [(30 if gap == 1 else 31, nxt)]
    out = []
    if gap > 0:
        out.append((7 if gap <= 8 else 8, nxt))
    out.append((value_token(v), z))
    return out


def value_bits(v, z, nxt, fb):
    """Their bits; fb [4][32]: code length + extra bits of each token in the AC groups of the block's plane."""
    return sum(fb[group(zs)][t] for t, zs in value_tokens(v, z, nxt))


def full_bits(bits):
    """enc_bqi_ref.token_bits' [4][32] code lengths with each token's extra bits added."""
    return [[int(bits[g][t]) + EXTRA_BITS[t] for t in range(32)] for g in range(4)]


def rate(lev, fb):
    """R: the AC tokens of the levels from index 1, the block's own EOB included (enc_bqi_ref.ac_bits, token by token)."""
    r, nxt = 0, 1
    for z in range(1, 64):
        if lev[z]:
            r += value_bits(int(lev[z]), z, nxt, fb)
            nxt = z + 1
    return r + (fb[group(nxt)][0] if nxt < 64 else 0)


def dist(c, lev, s):
    return sum((int(c[z]) - int(lev[z]) * int(s[z])) ** 2 for z in range(1, 64))


def _alt(v):
    return v - (1 if v > 0 else -1)


def choose_block(c, lev, s, fb, lam):
    """The rule by its backward programme.  c, lev, s: the block's fDCT, levels and steps (zig-zag, 64 each); lam = lambda_q.
    -> dict(lev (a list), jbefore, jafter, rate, zeroed, lowered)."""
    lev = [int(v) for v in lev]
    d0, r0 = dist(c, lev, s), rate(lev, fb)
    res = dict(lev=lev, jbefore=d0 + lam * r0, jafter=d0 + lam * r0, rate=r0, zeroed=0, lowered=0)
    nz = [z for z in range(1, 64) if lev[z]]
    if lam == 0 or not nz:
        return res
    dd = {z: (int(c[z]) - _alt(lev[z]) * int(s[z])) ** 2 - (int(c[z]) - lev[z] * int(s[z])) ** 2 for z in nz}
    F, ch = {}, {}
    for zi in reversed([0] + nz):
        best, bc, acc, is_open = None, None, 0, True
        for zj in (z for z in nz if z > zi):
            l = lev[zj]
            cost = acc + F[zj] + lam * value_bits(l, zj, zi + 1, fb)
            if best is None or cost < best:
                best, bc = cost, (zj, False)
            if abs(l) >= 2:
                cost = acc + F[zj] + dd[zj] + lam * value_bits(_alt(l), zj, zi + 1, fb)
                if cost < best:
                    best, bc = cost, (zj, True)
                is_open = False
                break
            acc += dd[zj]
        if is_open:
            cost = acc + (lam * fb[group(zi + 1)][0] if zi < 63 else 0)
            if best is None or cost < best:
                best, bc = cost, None
        F[zi], ch[zi] = best, bc
    out, z = list(lev), 0
    while True:
        nxt = ch[z]
        for zz in nz:
            if zz > z and (nxt is None or zz < nxt[0]):
                out[zz] = 0
                res["zeroed"] += 1
        if nxt is None:
            break
        if nxt[1]:
            out[nxt[0]] = _alt(lev[nxt[0]])
            res["lowered"] += 1
        z = nxt[0]
    res.update(lev=out, jafter=d0 + F[0], rate=rate(out, fb))
    return res


def brute_block(c, lev, s, fb, lam):
    """The rule by its words: every a in lexicographic order, the first of least J."""
    lev = [int(v) for v in lev]
    nz = [z for z in range(1, 64) if lev[z]]
    if lam == 0:
        return lev, dist(c, lev, s) + lam * rate(lev, fb)
    best = None
    for a in itertools.product((0, 1), repeat=len(nz)):
        cand = list(lev)
        for z, az in zip(nz, a):
            if az:
                cand[z] = _alt(lev[z])
        j = dist(c, cand, s) + lam * rate(cand, fb)
        if best is None or j < best[0]:
            best = (j, cand)
    return best[1], best[0]


def block_lambda_q(tab0, w, iscale=None, lam_fix=None):
    """lambda_q of a block whose table at qis[0] is tab0."""
    return (S.block_lambda(tab0, iscale, lam_fix) * int(w)) >> 4


def rdq_code(geo, src, prev, gold, fvx, fvy, qti, cls, coded, lev, qii, tabs, bits2, w, iscale=None, lam_fix=None):
    """The frame's blocks under the rule.  src, prev, gold: three planes each, bitstream rows (prev, gold None on a key frame); the
    rest in fragment raster order: fvx, fvy the vectors, qti (0 intra, 1 inter), cls (3: GOLD), coded, lev [nfrags, 64], qii; tabs: a
    list over the qi list of {(qti, plane): zig-zag steps}; bits2: (luma, chroma) [4][32] code lengths.
    -> dict(lev [nfrags, 64], jbefore, jafter, rate (raster, 0 for uncoded blocks), zeroed [3], lowered [3], emptied, rate_before,
    rate_after, dist_before, dist_after)."""
    out = dict(lev=np.array(lev, np.int64), jbefore=np.zeros(geo.nfrags, np.int64), jafter=np.zeros(geo.nfrags, np.int64),
               rate=np.zeros(geo.nfrags, np.int64), zeroed=[0] * 3, lowered=[0] * 3, emptied=0, rate_before=0, rate_after=0,
               dist_before=0, dist_after=0)
    fb2 = [full_bits(b) for b in bits2]
    r8 = np.arange(8)
    for p, g in enumerate(geo.planes):
        nh, o = g["nhfrags"], g["froffset"]
        qx, qy = p > 0 and geo.hdec, p > 0 and geo.vdec
        for loc in range(g["nfrags"]):
            f = o + loc
            if not coded[f]:
                continue
            Y, X = (loc // nh) * 8 + r8[:, None], (loc % nh) * 8 + r8[None, :]
            s = src[p][Y, X].astype(np.int64)
            t = int(qti[f])
            pred = 128 if t == 0 else IR.predict((gold if cls[f] == 3 else prev)[p], X, Y, int(fvx[f]), int(fvy[f]), qx, qy)
            c = oracle.fdct8x8_batch((s - pred).reshape(1, 64).astype(np.int16))[0]
            lam = block_lambda_q(tabs[0][(t, p)], w, None if iscale is None else iscale[f], lam_fix)
            steps = tabs[int(qii[f])][(t, p)]
            r = choose_block(c, lev[f], steps, fb2[int(p > 0)], lam)
            out["lev"][f] = r["lev"]
            out["jbefore"][f], out["jafter"][f], out["rate"][f] = r["jbefore"], r["jafter"], r["rate"]
            out["zeroed"][p] += r["zeroed"]
            out["lowered"][p] += r["lowered"]
            out["emptied"] += int(any(lev[f][1:]) and not any(r["lev"][1:]))
            r0 = rate(lev[f], fb2[int(p > 0)])
            out["rate_before"] += r0
            out["rate_after"] += r["rate"]
            out["dist_before"] += r["jbefore"] - lam * r0
            out["dist_after"] += r["jafter"] - lam * r["rate"]
    return out


def stage(geo, src, prev, gold, classes, pix, mv, bmv, dequant, bits, levels, qii, cmap, w, iscale=None, lam_fix=None):
    """rdq_code in thip_enc_rdq_stage's shapes: classes 0 (a key frame: pix, mv, bmv, cmap unused), 2 or 3; dequant [nqis][2][3][64];
    bits uint8 [2][4][32] (code length + extra bits); levels [nfrags, 64] and qii [nfrags] (or None) in CODED order; cmap raster.
    -> dict(levels [nfrags, 64] int16, jbefore, jafter, rate: coded order)."""
    from tests import enc_modes_ref as M
    dq = np.asarray(dequant, np.int64).reshape(-1, 2, 3, 64)
    tabs = [{(t, p): dq[k, t, p] for t in range(2) for p in range(3)} for k in range(dq.shape[0])]
    b = (np.asarray(bits, np.int64).reshape(2, 4, 32) - np.asarray(EXTRA_BITS, np.int64)[None, None, :]).tolist()
    co, nf = geo.coded_order, geo.nfrags
    lev = np.zeros((nf, 64), np.int64)
    lev[co] = np.asarray(levels, np.int64)
    q = np.zeros(nf, np.int64)
    if qii is not None:
        q[co] = np.minimum(np.asarray(qii, np.int64), dq.shape[0] - 1)
    if classes == 0:
        fvx = fvy = np.zeros(nf, np.int64)
        qti, cls, coded = np.zeros(nf, np.int64), np.ones(nf, np.int64), np.ones(nf, bool)
    else:
        pix, mv = np.asarray(pix, np.int64), np.asarray(mv, np.int64)
        bmv = np.zeros((len(pix), 4, 2), np.int64) if bmv is None else np.asarray(bmv, np.int64)
        fvx, fvy = M.fragment_vectors(geo, pix, mv, bmv)
        fvx, fvy, fpix = fvx.copy(), fvy.copy(), pix[geo.mb_of].copy()
        coded = np.asarray(cmap) != 0
        nh0 = geo.planes[0]["nhfrags"]
        for mb in range(len(pix)):   # a macro block none of whose luma blocks is coded is INTER_NOMV to the decoder
            f0 = 2 * (mb // geo.nmbx) * nh0 + 2 * (mb % geo.nmbx)
            if not coded[[f0, f0 + 1, f0 + nh0, f0 + nh0 + 1]].any():
                lost = (geo.mb_of == mb) & (geo.plane_of > 0)
                fpix[lost], fvx[lost], fvy[lost] = M.NOMV, 0, 0
        qti = np.where(fpix == M.INTRA, 0, 1)
        cls = np.where(qti == 0, 1, np.where((fpix == M.GOLDEN_NOMV) | (fpix == M.GOLDEN_MV), 3, 2))
    d = rdq_code(geo, src, prev, gold, fvx, fvy, qti, cls, coded, lev, q, tabs, b, w, iscale, lam_fix)
    return dict(levels=d["lev"][co].astype(np.int16), jbefore=d["jbefore"][co], jafter=d["jafter"][co], rate=d["rate"][co], detail=d)


# ---- the stream ----------------------------------------------------------------------------------------------------------------
STAT_FIELDS = ("zeroed", "lowered", "emptied", "rate_before", "rate_after", "dist_before", "dist_after")


class RdqEncoder(S.SkipEncoder):
    """The stream th_encode_* makes with TH_ENCCTL_THIP_SET_RD_QUANT = w (w = 0: SkipEncoder's stream).  frame() returns SkipEncoder's
    dict plus rdq (TH_ENCCTL_THIP_GET_RD_QUANT_STATS as Encoder.rd_quant_stats returns it, without rdq_ms) and, for a frame that went
    through the choice, rdq_changed: how many coded blocks it changed."""

    def __init__(self, fw, fh, fmt, pic, setup, kf_interval, shift, delta=0, k=0, modes=True, rd=False, skip=True, w=0):
        super().__init__(fw, fh, fmt, pic, setup, kf_interval, shift, delta, k, modes, rd, skip)
        self.w = w
        self._rdq = None

    def frame(self, planes, qi, dups=0):
        self._rdq = None
        self._planes = planes
        out = super().frame(planes, qi, dups)
        m = self._rdq if out["packet"] else None
        out["rdq"] = dict(weight=self.w, measured=int(m is not None), lam=m["lam"] if m else 0,
                          **{n: (m[n] if m else [0] * 3 if n in ("zeroed", "lowered") else 0) for n in STAT_FIELDS})
        if m:
            out["rdq_changed"] = m["changed"]
        return out

    def _finish(self, bw, lev, qii, qti_of, coded, cls, qis, key, qi):
        if not self.w:
            return super()._finish(bw, lev, qii, qti_of, coded, cls, qis, key, qi)
        geo, setup = self.geo, self.setup
        src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(self._planes, self.fw, self.fh, self.fmt, self.pic)]
        prev = gold = None
        if not key:
            prev = [self.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
            gold = [self.ost.get_plane(oracle.FRAME_GOLD, p) for p in range(3)]
        m = np.asarray(self.ost.mvs, np.int64)
        fvx, fvy = ((m & 0xFF) ^ 0x80) - 0x80, m >> 8
        iscale = None
        if self.k and self.delta:
            iscale = K.scales(K.activity(self._planes, self.fw, self.fh, self.fmt, self.pic), self.k, geo)[0]
        tabs = [{(t, p): setup.qmat(t, p, q)[ZIGZAG] for t in range(2) for p in range(3)} for q in qis]
        ht = self.hti[key]
        d = rdq_code(geo, src, prev, gold, fvx, fvy, qti_of, cls, coded, lev, qii, tabs,
                     [B.token_bits(setup, ht[0]), B.token_bits(setup, ht[1])], self.w, iscale)
        s1 = int(setup.qmat(0 if key else 1, 0, qi)[ZIGZAG][1])
        self._rdq = dict({n: d[n] for n in STAT_FIELDS}, lam=(s1 * s1 * B.LAM_NUM) >> B.LAM_SHIFT,
                         changed=int((d["lev"] != np.asarray(lev, np.int64)).any(1).sum()))
        return super()._finish(bw, d["lev"], qii, qti_of, coded, cls, qis, key, qi)


class CutRdqEncoder(RdqEncoder, S.R.enc_cut_ref.CutBase):
    """RdqEncoder with automatic key frames at ratio self.t."""


class RateStream(S.R.enc_rate_ref.RateStream):
    """enc_rate_ref's bitrate-mode stream with RdqEncoder: the probe and the controller are unchanged."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, fps=(30, 1), kf_interval=64, shift=6, delta=0, k=0, modes=True, rd=False,
                 skip=True, w=0, **kw):
        super().__init__(fw, fh, fmt, pic, setup, bitrate, fps=fps, inter=True, kf_interval=kf_interval, shift=shift, **kw)
        self.enc.close()
        self.enc = RdqEncoder(fw, fh, fmt, pic, setup, kf_interval, shift, delta, k, modes, rd, skip, w)


# ---- the packet cases of tests/test_gpu_encoder_rdq.py (tests/test_encoder_rdq_cpu.py asserts that they are not vacuous) ----------
# (clip kind, frame width, height, pixel format, quality, frames, key-frame interval, modes, block qi, masking, rd, skip, w)
PACKET_CASES = [("pan", 64, 48, 0, 32, 2, 1, False, 0, 0, False, False, 5), ("pan", 64, 48, 2, 32, 2, 1, False, 8, 4, False, False, 8),
                ("pan", 64, 48, 0, 32, 3, 64, False, 0, 0, False, False, 5), ("static", 64, 48, 3, 32, 3, 64, True, 0, 0, False, True, 5),
                ("pan", 64, 48, 2, 24, 3, 64, True, 8, 0, True, False, 16), ("static", 64, 48, 0, 40, 3, 64, False, 8, 4, False, True, 3),
                ("pan", 176, 144, 0, 32, 3, 64, True, 8, 4, True, True, 5)]


def case_frames(case):
    return S.clip(case[0], case[1], case[2], case[3], case[5], seed=case[4])


def case_encoder(case, setup, w=None):
    kind, fw, fh, fmt, q, nf, kf, modes, delta, k, rd, skip, cw = case
    return RdqEncoder(fw, fh, fmt, (0, 0, fw, fh), setup, kf, 6, delta, k, modes, rd, skip, cw if w is None else w)
