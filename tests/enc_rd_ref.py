"""enc_rd_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s rate-distortion mode decision (TH_ENCCTL_THIP_SET_RD_MODES;
include/theoraenc_hip.h, "Rate-distortion mode decision") in numpy, to compare the library's costs, words and packets with.  Integer
arithmetic throughout.

The search is tests/enc_modes_ref.search_all's, the transform and the quantiser the oracle's; what is new is the cost of every macro
block under each of six candidates and the choice of the least.  RdEncoder is tests/enc_mask_ref.MaskEncoder (and so
enc_bqi_ref.BqiEncoder) with that choice in place of enc_modes_ref.decide's: block qi and masking compose, and with both off the
stream is enc_modes_ref.ModesEncoder's but for the modes.
"""
import numpy as np

import oracle
from tests import enc_cut_ref, enc_rate_ref, enc_ref
from tests import enc_mask_ref as K
from tests import enc_modes_ref as M
from tests.enc_inter_ref import predict
from tests.enc_modes_ref import GOLDEN_MV, GOLDEN_NOMV, INTRA, MV, MV_FOUR, NOMV
from tests.enc_ref import ZIGZAG
from tests.packref import EXTRA_BITS

CANDS = (NOMV, MV, MV_FOUR, GOLDEN_NOMV, GOLDEN_MV, INTRA)   # the candidates, in the rule's order
LAM_NUM, LAM_SHIFT = 40, 7                                   # lambda = (s1 * s1 * 40) >> 7
HEADER_BITS = (1, 15, 55, 5, 18, 4)                          # H_m
FIRST_TABLE = 5                                              # every table index before an inter packet exists


def rd_lambda(s1):
    return (int(s1) * int(s1) * LAM_NUM) >> LAM_SHIFT


def bits_table(setup, hti):
    """uint8 [2][5][32]: luma then chroma, code length + extra bits of token tok in Huffman group hg, from the DC table hti[0 / 1]
    (group 0) and the AC table hti[2 / 3] (groups 1..4) -- what thip_enc_rd_stage takes as `bits`."""
    out = np.zeros((2, 5, 32), np.uint8)
    for c in range(2):
        for hg in range(5):
            codes = setup.codes[16 * hg + hti[(2 if hg else 0) + c]]
            for tok in range(32):
                out[c, hg, tok] = len(codes[tok]) + EXTRA_BITS[tok]
    return out


def _hg(z):
    return 0 if z == 0 else 1 if z <= 5 else 2 if z <= 14 else 3 if z <= 27 else 4


def _value_token(a):
    """The smallest value token of the non-zero value a (spec Table 7.38); the largest where none carries it."""
    aa = abs(a)
    if aa <= 2:
        return 7 + 2 * aa + (a < 0)
    return 10 + aa if aa <= 6 else 17 if aa <= 8 else 18 if aa <= 12 else 19 if aa <= 20 else 20 if aa <= 36 else 21 if aa <= 68 else 22


def block_bits(v, bits):
    """R of one block: the tokens of zig-zag values v (the charged DC at index 0) from index 0, the block's own EOB included; bits
    [5][32] of Python integers.  A value beyond the largest value token's range (|v| > 580) costs that token, as the device counts it."""
    r, nxt = 0, 0
    for z in np.flatnonzero(v):
        z = int(z)
        a, g = int(v[z]), z - nxt
        aa = abs(a)
        if aa == 1 and 1 <= g <= 17:
            r += bits[_hg(nxt)][22 + g if g <= 5 else 28 if g <= 9 else 29]
        elif aa in (2, 3) and 1 <= g <= 3:
            r += bits[_hg(nxt)][30 if g == 1 else 31]
        else:
            if g > 0:
                r += bits[_hg(nxt)][7 if g <= 8 else 8]
            r += bits[_hg(z)][_value_token(a)]
        nxt = z + 1
    if nxt < 64:
        r += bits[_hg(nxt)][0]
    return int(r)


def candidate(ms, m):
    """Candidate m of every macro block as enc_modes_ref.decide hands a decision out: (pix [nmbs], mv [nmbs, 2], bmv [nmbs, 4, 2])."""
    n = len(ms["s0"])
    pix = np.full(n, CANDS[m], np.int64)
    mv = np.zeros((n, 2), np.int64)
    bmv = np.zeros((n, 4, 2), np.int64)
    if CANDS[m] == MV:
        mv = np.stack([ms["mvx"], ms["mvy"]], 1).astype(np.int64)
    elif CANDS[m] == GOLDEN_MV:
        mv = np.stack([ms["gvx"], ms["gvy"]], 1).astype(np.int64)
    elif CANDS[m] == MV_FOUR:
        bmv = np.stack([ms["bvx"], ms["bvy"]], 2).astype(np.int64)
    return pix, mv, bmv


def block_costs(geo, src, prev, gold, ms, tabs, bits, lam, m):
    """Per fragment (raster) under candidate m: (D_b + lambda R_b with the NOMV exception applied [nfrags], D_b, R_b, levels, dct)."""
    pix, mv, bmv = candidate(ms, m)
    fvx, fvy = M.fragment_vectors(geo, pix, mv, bmv)
    intra = CANDS[m] == INTRA
    ref = gold if CANDS[m] in (GOLDEN_NOMV, GOLDEN_MV) else prev
    nf = geo.nfrags
    D, R, cost = np.zeros(nf, np.int64), np.zeros(nf, np.int64), np.zeros(nf, np.int64)
    lev, dct = np.zeros((nf, 64), np.int64), np.zeros((nf, 64), np.int64)
    for p, g in enumerate(geo.planes):
        nh = g["nhfrags"]
        fi = g["froffset"] + np.arange(g["nfrags"])
        fy, fx = (fi - g["froffset"]) // nh, (fi - g["froffset"]) % nh
        r = np.arange(8)
        Y = fy[:, None, None] * 8 + r[None, :, None]
        X = fx[:, None, None] * 8 + r[None, None, :]
        if intra:
            pred = 128
        else:
            pred = predict(ref[p], X, Y, fvx[fi][:, None, None], fvy[fi][:, None, None], p > 0 and geo.hdec, p > 0 and geo.vdec)
        c = oracle.fdct8x8_batch((src[p][Y, X] - pred).reshape(-1, 64).astype(np.int16))
        tab = np.asarray(tabs[(0 if intra else 1, p)], np.int64)
        q = oracle.quantize_batch(c, tab.astype(np.uint16))[0].astype(np.int64)
        c = c.astype(np.int64)
        e = c - q * tab
        D[fi] = (e * e).sum(1)
        lev[fi], dct[fi] = q, c
        charged = q.copy()
        if intra and p == 0:   # luma blocks 1..3 of a macro block: less block 0's quantised DC
            first = (fy & ~1) * nh + (fx & ~1)
            sub = (fy & 1) | (fx & 1)
            charged[sub != 0, 0] -= q[first[sub != 0], 0]
        b5 = np.asarray(bits, np.int64)[int(p > 0)].tolist()   # (Python integers: a uint8 sum would wrap)
        for k in range(len(fi)):
            R[fi[k]] = block_bits(charged[k], b5)
        cost[fi] = D[fi] + lam * R[fi]
        if CANDS[m] == NOMV:   # an uncoded block: no bits, the whole residual
            zero = ~(q != 0).any(1)
            cost[fi[zero]] = (c[zero] * c[zero]).sum(1)
    return cost, D, R, lev, dct


def rd_costs(geo, src, prev, gold, ms, tabs, bits, lam):
    """J [nmbs, 6] (int64): every macro block's cost under every candidate.  src, prev, gold: three planes each, bitstream rows; ms:
    enc_modes_ref.search_all's dict; tabs[(qti, plane)]: zig-zag steps; bits: bits_table's [2][5][32]; lam: the rule's lambda."""
    n = len(ms["s0"])
    J = np.zeros((n, 6), np.int64)
    for m in range(6):
        cost = block_costs(geo, src, prev, gold, ms, tabs, bits, lam, m)[0]
        np.add.at(J[:, m], geo.mb_of, cost)
        J[:, m] += lam * HEADER_BITS[m]
    return J


def rd_decide(ms, J):
    """The least J a macro block, a tie to the lower index, as enc_modes_ref.decide hands a decision out (pix, mv, bmv), plus cand
    (the winning index) and J."""
    best = np.argmin(J, axis=1)   # (the first of equal minima)
    pix = np.asarray(CANDS, np.int64)[best]
    n = len(best)
    mv = np.zeros((n, 2), np.int64)
    mv[pix == MV] = np.stack([ms["mvx"], ms["mvy"]], 1)[pix == MV]
    mv[pix == GOLDEN_MV] = np.stack([ms["gvx"], ms["gvy"]], 1)[pix == GOLDEN_MV]
    bmv = np.zeros((n, 4, 2), np.int64)
    bmv[pix == MV_FOUR] = np.stack([ms["bvx"], ms["bvy"]], 2)[pix == MV_FOUR]
    return dict(ms, pix=pix, mv=mv, bmv=bmv, cand=best, J=J)


# ---- the words of thip_enc_rd_stage --------------------------------------------------------------------------------------------
def _pk(x, y):
    return (np.asarray(x, np.int64) & 0xFF) | (np.asarray(y, np.int64) & 0xFF) << 8


def pack_cand(ms):
    """k_enc_me_cand's records [nmbs, 8] (uint32)."""
    z = np.zeros(len(ms["s0"]), np.int64)
    bv = [_pk(ms["bvx"][:, k], ms["bvy"][:, k]) for k in range(4)]
    return np.stack([_pk(ms["mvx"], ms["mvy"]) | _pk(ms["gvx"], ms["gvy"]) << 16, bv[0] | bv[1] << 16, bv[2] | bv[3] << 16,
                     ms["s0"] | ms["smv"] << 16, ms["s4"] | ms["si"] << 16, ms["g0"] | ms["gmv"] << 16, z, z], 1).astype(np.uint32)


def pack_words(d):
    """k_enc_me_all's words [nmbs, 4] of a decision (rd_decide's, or enc_modes_ref.decide's)."""
    from tests import inter_stage_ref
    return inter_stage_ref.pack_words8(d["pix"], d["mv"], d["bmv"], np.stack([d["gvx"], d["gvy"]], 1))


# ---- the packet cases of tests/test_gpu_encoder_rd.py (tests/test_encoder_rd_cpu.py asserts that they are not vacuous) -----------------
# (enc_modes_ref.sequence kind, frame width, height, pixel format, quality, frames); the sequence's seed is the quality
PACKET_CASES = [("uncover", 64, 48, 0, 48, 4), ("uncover", 80, 64, 2, 16, 4), ("uncover", 64, 48, 3, 0, 4), ("pan", 176, 144, 0, 16, 3),
                ("cut", 80, 64, 2, 63, 4), ("cut", 64, 48, 3, 48, 4), ("uncover", 96, 64, 0, 0, 4), ("pan", 80, 64, 3, 0, 3)]


def case_frames(case):
    kind, w, h, fmt, q, nf = case
    return M.sequence(kind, w, h, fmt, nf, seed=q)


# ---- the stream ----------------------------------------------------------------------------------------------------------------
class RdEncoder(K.MaskEncoder):
    """The stream th_encode_* makes with eight modes and TH_ENCCTL_THIP_SET_RD_MODES on (rd=False: off), block qi `delta` and masking
    `k` (0: off).  frame() returns MaskEncoder's dict plus rd (TH_ENCCTL_THIP_GET_RD_STATS as Encoder.rd_stats returns it, without
    rd_ms) and, for a frame decided by the rule, decision (rd_decide's dict)."""

    def __init__(self, fw, fh, fmt, pic, setup, kf_interval, shift, delta=0, k=0, modes=True, rd=True, lam_num=LAM_NUM, header_bits=HEADER_BITS):
        super().__init__(fw, fh, fmt, pic, setup, kf_interval, shift, delta, k, modes)
        self.rd, self.lam_num, self.header_bits = rd, lam_num, tuple(header_bits)
        self.rd_hti = [FIRST_TABLE] * 4
        self._rd = None

    def frame(self, planes, qi, dups=0):
        self._rd = None
        out = super().frame(planes, qi, dups)
        m = self._rd if out["packet"] else None
        out["rd"] = dict(on=int(self.rd), measured=int(m is not None), huff=m["huff"] if m else [0] * 4, lam=m["lam"] if m else 0)
        if m:
            out["decision"] = m["decision"]
        return out

    def _inter(self, planes, qi):
        if not (self.rd and self.modes):
            out = super()._inter(planes, qi)
        else:
            geo, setup = self.geo, self.setup
            src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]
            prev = [self.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
            gold = [self.ost.get_plane(oracle.FRAME_GOLD, p) for p in range(3)]
            tabs = {(t, p): setup.qmat(t, p, qi)[ZIGZAG] for t in range(2) for p in range(3)}
            s1 = int(tabs[(1, 0)][1])
            lam = (s1 * s1 * self.lam_num) >> LAM_SHIFT
            ms = M.search_all(src[0], prev[0], gold[0])
            J = _rd_costs_h(geo, src, prev, gold, ms, tabs, bits_table(setup, self.rd_hti), lam, self.header_bits)
            d = rd_decide(ms, J)
            self._rd = dict(huff=list(self.rd_hti), lam=lam, decision=d)
            # ModesEncoder._inter and BqiEncoder._inter look the search up in enc_modes_ref at call time: hand them the decision
            saved = M.motion_search
            M.motion_search = lambda *a: d
            try:
                out = super()._inter(planes, qi)
            finally:
                M.motion_search = saved
        if out["packet"]:
            self.rd_hti = [int(v) for v in out["huff"]]
        return out


def _rd_costs_h(geo, src, prev, gold, ms, tabs, bits, lam, header_bits):
    """rd_costs with other header bits (the tuning of DESIGN.md section 5.16)."""
    J = rd_costs(geo, src, prev, gold, ms, tabs, bits, lam)
    return J + lam * (np.asarray(header_bits, np.int64) - np.asarray(HEADER_BITS, np.int64))[None, :]


class CutRdEncoder(RdEncoder, enc_cut_ref.CutBase):
    """RdEncoder with automatic key frames at ratio self.t."""


class RateStream(enc_rate_ref.RateStream):
    """enc_rate_ref's bitrate-mode stream with RdEncoder: the probe and the controller are unchanged, the frames are coded at the
    chosen qi with the rule's modes."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, fps=(30, 1), kf_interval=64, shift=6, delta=0, k=0, **kw):
        super().__init__(fw, fh, fmt, pic, setup, bitrate, fps=fps, inter=True, kf_interval=kf_interval, shift=shift, **kw)
        self.enc.close()
        self.enc = RdEncoder(fw, fh, fmt, pic, setup, kf_interval, shift, delta, k)
