"""enc_bqi_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s block-level qi (TH_ENCCTL_THIP_SET_BLOCK_QI;
include/theoraenc_hip.h, "Block-level qi") in numpy, to compare the library's packets with byte for byte.  Integer arithmetic
throughout.

It codes key frames and inter frames with five or eight modes.  The searches and the mode rules are tests/enc_inter_ref.py's and
tests/enc_modes_ref.py's, the transform and the quantiser the oracle's, the token writer enc_inter_ref's; the reference is the oracle's
decode of the packets restated so far, so the restatement also states the reconstruction the encoder must reach.  What is new: the
frame's qi list, the per-block choice, the qii flags and the per-block AC dequantisation.
"""
import numpy as np

import oracle
from tests import enc_inter_ref as IR
from tests import enc_modes_ref as M
from tests import enc_ref
from tests.enc_inter_ref import mode_bits, mv_vlc_bits, token_packet_tail
from tests.enc_modes_ref import GOLDEN_MV, GOLDEN_NOMV, INTRA, MV, MV_FOUR, MV_LAST, MV_LAST2, NOMV
from tests.enc_ref import ZIGZAG, block_tokens
from tests.streamgen import MODE_ALPHABETS, MODE_REFI, BitWriter, write_long_runs, write_mv, write_short_runs

LAM_NUM, LAM_SHIFT = 40, 7   # lambda = (s * s * 40) >> 7
FLAG_BIAS = 1                # lambda x this many bits against k != 0
FIRST_TABLE = 5              # the AC table index before a packet of the frame type exists


def qi_list(qi, delta):
    """The frame's qi list: qi, then qi - delta (clamped at 0) and qi + delta (clamped at 63), each only when new."""
    qis = [qi]
    if delta:
        coarse, fine = max(qi - delta, 0), min(qi + delta, 63)
        if coarse != qi:
            qis.append(coarse)
        if fine != qi and fine != coarse:
            qis.append(fine)
    return qis


def token_bits(setup, t):
    """[4][32]: the code length of token tok in table t of Huffman group hg + 1 (hg = 0..3)."""
    return [[len(setup.codes[16 * (hg + 1) + t].get(tok, "")) for tok in range(32)] for hg in range(4)]


def ac_bits(lv, bits):
    """R: the bits of a block's AC tokens (zig-zag levels lv): the walk starts at index 1 (the DC counts as not zero), the block's own
    EOB included; each token its code length in the table of its start index's group, plus its extra bits."""
    v = np.array(lv, np.int64)
    v[0] = 1
    r = 0
    for t in block_tokens(v)[1:]:
        hg = enc_ref.huff_group(t[0]) - 1
        r += bits[hg][0] if t[1] == "EOB" else bits[hg][t[1]] + t[3]
    return r


def choose(dct, tabs, bits, bias=FLAG_BIAS):
    """The choice for blocks of one table: dct [n, 64] the fDCT (oracle.fdct8x8_batch: zig-zag order), tabs the table at each qi of
    the list (zig-zag), bits token_bits of the block's plane.  Returns (levels [n, 64] zig-zag with the DC at qis[0], qii [n])."""
    levs, dist = [], []
    c = dct.astype(np.int64)
    for tab in tabs:
        q, _ = oracle.quantize_batch(dct, np.asarray(tab, np.uint16))
        q = q.astype(np.int64)
        levs.append(q)
        e = c[:, 1:] - q[:, 1:] * np.asarray(tab, np.int64)[1:]
        dist.append((e * e).sum(1))
    s = int(tabs[0][1])
    lam = (s * s * LAM_NUM) >> LAM_SHIFT
    n = dct.shape[0]
    qii = np.zeros(n, np.int64)
    out = levs[0].copy()
    for i in range(n):
        best = None
        for k in range(len(tabs)):
            j = int(dist[k][i]) + lam * (ac_bits(levs[k][i], bits) + (bias if k else 0))
            if best is None or j < best:
                best, qii[i] = j, k
        if qii[i]:
            out[i, 1:] = levs[qii[i]][i, 1:]
    return out, qii


class BqiEncoder(M.ModesEncoder):
    """The stream th_encode_* makes with TH_ENCCTL_THIP_SET_BLOCK_QI = delta: intra-only (kf_interval 1), inter frames with five modes
    (modes=False) or eight (modes=True).  frame() returns enc_modes_ref's dict plus bqi (TH_ENCCTL_THIP_GET_BLOCK_QI_STATS as
    Encoder.block_qi_stats returns it) and qii (coded order, over all blocks)."""

    def __init__(self, fw, fh, fmt, pic, setup, kf_interval, shift, delta, modes=False, bias=FLAG_BIAS):
        super().__init__(fw, fh, fmt, pic, setup, kf_interval, shift)
        self.delta, self.modes, self.bias = delta, modes, bias
        self.hti = {True: (FIRST_TABLE, FIRST_TABLE), False: (FIRST_TABLE, FIRST_TABLE)}   # AC luma, chroma of the last packet a type

    def frame(self, planes, qi, dups=0):
        out = super().frame(planes, qi, dups)
        if not out["packet"]:
            out["bqi"] = dict(nqis=0, qis=[0, 0, 0], blocks=[[0] * 3 for _ in range(3)], flag_bits=0)
        return out

    def _code(self, src, pred, intra, qis, key):
        """Residual, transform, choice per block (raster order): (levels [nfrags, 64], qii [nfrags], qti [nfrags])."""
        geo, setup = self.geo, self.setup
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
            bits = token_bits(setup, ht[int(p > 0)])
            for t in range(2):
                sel = qti_of[fi] == t
                if sel.any():
                    tabs = [setup.qmat(t, p, q)[ZIGZAG] for q in qis]
                    lev[fi[sel]], qii[fi[sel]] = choose(dct[sel], tabs, bits, self.bias)
        return lev, qii, qti_of

    @staticmethod
    def _qii_flags(bw, qii_coded, nqis):
        """Spec 7.6 over the coded blocks' qii (coded order)."""
        if nqis < 2:
            return
        write_long_runs(bw, [int(q > 0) for q in qii_coded])
        if nqis == 3 and any(q > 0 for q in qii_coded):
            write_long_runs(bw, [int(q > 1) for q in qii_coded if q > 0])

    def _finish(self, bw, lev, qii, qti_of, coded, cls, qis, key, qi):
        """Qii flags, tokens, the oracle's reconstruction (modes, vectors already in self.ost); the stats."""
        geo, setup = self.geo, self.setup
        cf = geo.coded_order[coded[geo.coded_order]]
        nqis = len(qis)
        nb0 = len(bw.bits)
        self._qii_flags(bw, qii[cf], nqis)
        flag_bits = len(bw.bits) - nb0
        dcr = M.dc_residuals(geo, lev, coded, cls, 3)
        vals = lev[cf].copy()
        vals[:, 0] = dcr[cf]
        hti, ntok, nmerged, last_zzi = token_packet_tail(bw, vals, geo.plane_of[cf], setup)
        self.hti[key] = (hti[2], hti[3])
        tabs = {(t, p, k): setup.qmat(t, p, q)[ZIGZAG] for t in range(2) for p in range(3) for k, q in enumerate(qis)}
        dq = np.stack([tabs[(int(qti_of[f]), int(geo.plane_of[f]), int(qii[f]))] for f in cf])
        dc = np.array([tabs[(int(qti_of[f]), int(geo.plane_of[f]), 0)][0] for f in cf], np.int64)
        coeffs = np.zeros((len(cf), 64), np.int64)
        coeffs[:, ZIGZAG] = lev[cf] * dq
        coeffs[:, 0] = lev[cf, 0]
        ncoded = [int(coded[geo.froff[p]:geo.froff[p] + g["nfrags"]].sum()) for p, g in enumerate(geo.planes)]
        unc = geo.coded_order[~coded[geo.coded_order]]
        self.ost.decode_frame(frame_type=0 if key else 1, coded_fragis=cf, ncoded=ncoded, coeffs=coeffs.astype(np.int16),
                              last_zzi=last_zzi, dc_quant=dc.astype(np.uint16), uncoded_fragis=unc, flimit=setup.lflims[qi])
        blocks = [[0] * 3 for _ in range(3)]
        for f in cf:
            blocks[int(qii[f])][int(geo.plane_of[f])] += 1
        bqi = dict(nqis=nqis, qis=list(qis) + [0] * (3 - nqis), blocks=blocks, flag_bits=flag_bits)
        return dict(packet=bw.bytes(), huff=hti, tokens=ntok, tokens_merged=nmerged, coded_fragis=cf, bqi=bqi, coded=ncoded,
                    qii=qii[geo.coded_order])

    def _header(self, bw, key, qis):
        bw.write(0, 1)
        bw.write(0 if key else 1, 1)
        bw.write(qis[0], 6)
        for q in qis[1:]:
            bw.write(1, 1)
            bw.write(q, 6)
        if len(qis) < 3:
            bw.write(0, 1)

    def _key(self, planes, qi):
        geo = self.geo
        qis = qi_list(qi, self.delta)
        src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]
        lev, qii, qti_of = self._code(src, [128] * 3, np.ones(geo.nfrags, bool), qis, True)
        bw = BitWriter()
        self._header(bw, True, qis)
        bw.write(0, 3)
        coded = np.ones(geo.nfrags, bool)
        ost = self.ost
        ost.coded[:] = 1
        ost.refi[:] = 2
        ost.mvs[:] = 0
        out = self._finish(bw, lev, qii, qti_of, coded, np.ones(geo.nfrags, np.int64), qis, True, qi)
        nmbs = len(geo.mb_order)
        out.update(modes=[0, nmbs, 0, 0, 0], mode_scheme=-1, mv_scheme=-1)
        return out

    def _inter(self, planes, qi):
        geo, setup = self.geo, self.setup
        qis = qi_list(qi, self.delta)
        src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]
        prev = [self.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
        gold = [self.ost.get_plane(oracle.FRAME_GOLD, p) for p in range(3)]
        lam = int(setup.qmat(1, 0, qi)[ZIGZAG][1])
        if self.modes:
            ms = M.motion_search(src[0], prev[0], gold[0], lam)
            pix, mv, bmv = ms["pix"], ms["mv"], ms["bmv"]
        else:
            pix, mvx, mvy = IR.motion_search(src[0], prev[0], lam)[:3]
            mv = np.stack([mvx, mvy], 1)
            bmv = np.zeros((len(pix), 4, 2), np.int64)
        fvx, fvy = M.fragment_vectors(geo, pix, mv, bmv)
        fpix = pix[geo.mb_of]
        fgold = (fpix == GOLDEN_NOMV) | (fpix == GOLDEN_MV)
        intra = fpix == INTRA
        preds = []
        for p, g in enumerate(geo.planes):
            nh = g["nhfrags"]
            fi = g["froffset"] + np.arange(g["nfrags"])
            fy, fx = (fi - g["froffset"]) // nh, (fi - g["froffset"]) % nh
            r = np.arange(8)
            Y = fy[:, None, None] * 8 + r[None, :, None]
            X = fx[:, None, None] * 8 + r[None, None, :]
            qx, qy = p > 0 and geo.hdec, p > 0 and geo.vdec
            vx, vy = fvx[fi][:, None, None], fvy[fi][:, None, None]
            pred = np.where(fgold[fi][:, None, None], IR.predict(gold[p], X, Y, vx, vy, qx, qy),
                            IR.predict(prev[p], X, Y, vx, vy, qx, qy))
            pred[intra[fi]] = 128
            preds.append(pred)
        lev, qii, qti_of = self._code(src, preds, intra, qis, False)
        cls = np.where(qti_of == 0, 1, np.where(fgold, 3, 2))
        coded = (fpix != NOMV) | (lev != 0).any(1)
        if not coded.any():
            return dict(packet=b"", modes=[0] * 5, coded=[0, 0, 0], mode_scheme=-1, mv_scheme=-1)
        bw = BitWriter()
        self._header(bw, False, qis)
        # 7.3 coded flags
        sbp, sbf, blk, at = [], [], [], 0
        for n in geo.sb_len:
            c = coded[geo.coded_order[at:at + n]]
            partial = 0 < c.sum() < n
            sbp.append(int(partial))
            if partial:
                blk.extend(int(v) for v in c)
            else:
                sbf.append(int(c.all()))
            at += n
        write_long_runs(bw, sbp)
        write_long_runs(bw, sbf)
        write_short_runs(bw, blk)
        # 7.4 modes, 7.5 vectors
        nh0 = geo.planes[0]["nhfrags"]
        modes, mvs, last1, last2 = [], [], (0, 0), (0, 0)
        counts = [0] * 8
        mb_mode = np.full(len(pix), NOMV)
        for mb in geo.mb_order:
            f0 = 2 * (mb // geo.nmbx) * nh0 + 2 * (mb % geo.nmbx)
            if not (coded[f0] or coded[f0 + 1] or coded[f0 + nh0] or coded[f0 + nh0 + 1]):
                counts[NOMV] += 1
                continue
            mode = int(pix[mb])
            if mode == MV:
                v = (int(mv[mb, 0]), int(mv[mb, 1]))
                if v == last1:
                    mode = MV_LAST
                elif v == last2:
                    mode = MV_LAST2
                    last2, last1 = last1, v
                else:
                    mvs.append(v)
                    last2, last1 = last1, v
            elif mode == MV_FOUR:
                for k in range(4):
                    mvs.append((int(bmv[mb, k, 0]), int(bmv[mb, k, 1])))
                last2, last1 = last1, mvs[-1]
            elif mode == GOLDEN_MV:
                mvs.append((int(mv[mb, 0]), int(mv[mb, 1])))
            modes.append(mode)
            mb_mode[mb] = mode
            counts[mode] += 1
        freq = [modes.count(m) for m in range(8)]
        alpha0 = sorted(range(8), key=lambda m: -freq[m])
        rank0 = [alpha0.index(m) for m in range(8)]
        scheme = int(np.argmin([mode_bits(freq, s, rank0) for s in range(8)]))
        bw.write(scheme, 3)
        if scheme == 0:
            for m in range(8):
                bw.write(rank0[m], 3)
        for m in modes:
            if scheme == 7:
                bw.write(m, 3)
            else:
                i = rank0[m] if scheme == 0 else MODE_ALPHABETS[scheme - 1].index(m)
                bw.code("1" * i + ("0" if i < 7 else ""))
        vlc = sum(mv_vlc_bits(c) for v in mvs for c in v)
        mvmode = 1 if vlc > 6 * 2 * len(mvs) else 0
        bw.write(mvmode, 1)
        for v in mvs:
            write_mv(bw, v[0], mvmode)
            write_mv(bw, v[1], mvmode)
        ost = self.ost
        ost.coded[:] = coded
        refi = np.array([MODE_REFI[int(m)] for m in mb_mode[geo.mb_of]], np.uint8)
        refi[~coded] = 3
        ost.refi[:] = refi
        ost.mvs[:] = ((fvx & 0xFF) | (fvy << 8)).astype(np.int16)
        out = self._finish(bw, lev, qii, qti_of, coded, cls, qis, False, qi)
        out.update(modes=counts[:5], modes8=counts, vectors=len(mvs), mode_scheme=scheme, mv_scheme=mvmode, pix=pix)
        return out
