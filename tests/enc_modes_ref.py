"""enc_modes_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s inter frames with all eight macro-block modes
(TH_ENCCTL_THIP_SET_INTER_MODES; include/theoraenc_hip.h, "All eight modes") in numpy, to compare the library's packets with byte
for byte.

It extends tests/enc_inter_ref.py: key frames, the reference (the oracle's decode of the packets restated so far), the transform,
the quantiser and the token writer are that restatement's.  What is new: a second reference (the oracle's GOLD frame), a search per
8 x 8 luma block, the eight-mode decision, the derived chroma vectors of INTER_MV_FOUR and three DC reference classes.
"""
import numpy as np

import oracle
from tests import enc_inter_ref as IR
from tests import enc_rate_ref, enc_ref
from tests.enc_inter_ref import mode_bits, mv_vlc_bits, predict, token_packet_tail
from tests.enc_ref import ZIGZAG
from tests.streamgen import MODE_ALPHABETS, MODE_REFI, BitWriter, write_long_runs, write_mv, write_short_runs

NOMV, INTRA, MV, MV_LAST, MV_LAST2, GOLDEN_NOMV, GOLDEN_MV, MV_FOUR = range(8)
MODE_NAMES = ("INTER_NOMV", "INTRA", "INTER_MV", "INTER_MV_LAST", "INTER_MV_LAST2", "GOLDEN_NOMV", "GOLDEN_MV", "INTER_MV_FOUR")
_KEYMAX = np.iinfo(np.int64).max


def round_div(v, shift):
    """The decoder's round(v / 2^shift), ties away from zero (thip_frontend.cpp round_div, spec 7.5.2)."""
    v = np.asarray(v, np.int64)
    half = 1 << (shift - 1)
    return np.where(v >= 0, (v + half) >> shift, -((-v + half) >> shift))


def full_pel(s, ref, blocks):
    """Full-pel search of every macro block of luma s (bitstream rows) against ref over [-15, 15]^2: the least key (SAD << 32 |
    2 (|dx| + |dy|) << 16 | raster index) per macro block [nmbs], per luma block in mb.luma order [nmbs, 4] (when blocks), and S0."""
    H, W = s.shape
    nmy, nmx = H // 16, W // 16
    pad = np.pad(ref, 16, mode="edge").astype(np.int64)
    best = np.full(nmy * nmx, _KEYMAX)
    bbest = np.full((nmy * nmx, 4), _KEYMAX) if blocks else None
    s0 = None
    for ci in range(31 * 31):
        dy, dx = ci // 31 - 15, ci % 31 - 15
        d = np.abs(s - pad[16 + dy:16 + dy + H, 16 + dx:16 + dx + W]).reshape(nmy, 2, 8, nmx, 2, 8).sum((2, 5))
        d = d.transpose(0, 2, 1, 3).reshape(nmy * nmx, 4)   # block k = 2 i + j: i the row (from the bottom), j the column
        tail = ((2 * (abs(dx) + abs(dy))) << 16) | ci
        mb = d.sum(1)
        best = np.minimum(best, (mb << 32) | tail)
        if blocks:
            bbest = np.minimum(bbest, (d << 32) | tail)
        if dx == 0 and dy == 0:
            s0 = mb
    return best, bbest, s0


def half_pel(s, ref, best, x0, y0, size):
    """The half-pel refinement of full-pel keys best [n] of the size x size blocks at (x0, y0): (SAD, mvx, mvy) arrays."""
    bci = best & 0xFFFF
    bdx, bdy = bci % 31 - 15, bci // 31 - 15
    r = np.arange(size)
    Y = y0[:, None, None] + r[None, :, None]
    X = x0[:, None, None] + r[None, None, :]
    sblk = s[Y, X]
    cur = (best >> 16 << 16) | 4
    for k9 in (0, 1, 2, 3, 5, 6, 7, 8):
        mvx, mvy = 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1
        p = predict(ref, X, Y, mvx[:, None, None], mvy[:, None, None], False, False)
        sad = np.abs(sblk - p).sum((1, 2))
        cur = np.minimum(cur, (sad << 32) | ((np.abs(mvx) + np.abs(mvy)) << 16) | k9)
    k9 = cur & 0xFFFF
    return cur >> 32, 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1


def intra_sad(s):
    """SI of every macro block of luma s (bitstream rows): the SAD of its four luma blocks against their rounded means."""
    H, W = s.shape
    n = (H // 16) * (W // 16)
    y0 = (np.arange(n) // (W // 16)) * 16
    x0 = (np.arange(n) % (W // 16)) * 16
    blk = s[(y0[:, None, None] + np.arange(16)[None, :, None]), (x0[:, None, None] + np.arange(16)[None, None, :])]
    b4 = blk.reshape(-1, 2, 8, 2, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 4, 64)
    return np.abs(b4 - ((b4.sum(2) + 32) >> 6)[:, :, None]).sum((1, 2))


def search_all(src, prev, gold):
    """Everything of the eight-mode search that does not depend on lambda, for every macro block (raster, rows from the bottom):
    a dict of the SADs (s0, smv, s4, g0, gmv, si) and the vectors found (mvx, mvy; gvx, gvy; bvx, bvy [nmbs, 4])."""
    H, W = src.shape
    nmy, nmx = H // 16, W // 16
    n = nmy * nmx
    s = src.astype(np.int64)
    y0 = (np.arange(n) // nmx) * 16
    x0 = (np.arange(n) % nmx) * 16
    best, bbest, s0 = full_pel(s, prev, True)
    smv, mvx, mvy = half_pel(s, prev, best, x0, y0, 16)
    bx0 = (x0[:, None] + 8 * (np.arange(4) & 1)[None, :]).reshape(-1)
    by0 = (y0[:, None] + 8 * (np.arange(4) >> 1)[None, :]).reshape(-1)
    sb, bvx, bvy = half_pel(s, prev, bbest.reshape(-1), bx0, by0, 8)
    s4 = sb.reshape(n, 4).sum(1)
    gbest, _, g0 = full_pel(s, gold, False)
    gmv, gvx, gvy = half_pel(s, gold, gbest, x0, y0, 16)
    return dict(s0=s0, smv=smv, s4=s4, g0=g0, gmv=gmv, si=intra_sad(s), mvx=mvx, mvy=mvy, gvx=gvx, gvy=gvy,
                bvx=bvx.reshape(n, 4), bvy=bvy.reshape(n, 4))


def decide(ms, lam):
    """The eight-mode decision of theoraenc_hip.h over search_all's dict: it gains pix (the pixel mode: NOMV, INTRA, MV,
    GOLDEN_NOMV, GOLDEN_MV or MV_FOUR), mv [nmbs, 2] (the vector of MV or GOLDEN_MV, else 0) and bmv [nmbs, 4, 2] (the block
    vectors of MV_FOUR, else 0); margins: left side less right side of the cascade's five inequalities, in its order."""
    s0, smv, s4, g0, gmv, si = (ms[k] for k in ("s0", "smv", "s4", "g0", "gmv", "si"))
    n = len(s0)
    # 1. PREV, one vector
    mv_win = smv + lam < s0
    pix = np.where(mv_win, MV, NOMV)
    C = np.where(mv_win, smv + lam, s0)
    S = np.where(mv_win, smv, s0)
    # 2. four vectors
    C1 = C
    four = s4 + 4 * lam < C
    pix, C, S = np.where(four, MV_FOUR, pix), np.where(four, s4 + 4 * lam, C), np.where(four, s4, S)
    # 3. GOLD
    gmv_win = gmv + 2 * lam < g0 + lam
    gpix = np.where(gmv_win, GOLDEN_MV, GOLDEN_NOMV)
    CG = np.where(gmv_win, gmv + 2 * lam, g0 + lam)
    SG = np.where(gmv_win, gmv, g0)
    gw = CG < C
    pix, S = np.where(gw, gpix, pix), np.where(gw, SG, S)
    # 4. INTRA
    margins = [smv + lam - s0, s4 + 4 * lam - C1, gmv + 2 * lam - (g0 + lam), CG - C, si + 4 * lam - S]
    pix = np.where(si + 4 * lam < S, INTRA, pix)
    mv = np.zeros((n, 2), np.int64)
    mv[pix == MV] = np.stack([ms["mvx"], ms["mvy"]], 1)[pix == MV]
    mv[pix == GOLDEN_MV] = np.stack([ms["gvx"], ms["gvy"]], 1)[pix == GOLDEN_MV]
    bmv = np.zeros((n, 4, 2), np.int64)
    bmv[pix == MV_FOUR] = np.stack([ms["bvx"], ms["bvy"]], 2)[pix == MV_FOUR]
    return dict(ms, pix=pix, mv=mv, bmv=bmv, margins=margins)


def motion_search(src, prev, gold, lam):
    """The eight-mode search and decision of every macro block (raster, rows from the bottom): decide over search_all."""
    return decide(search_all(src, prev, gold), lam)


def fragment_vectors(geo, pix, mv, bmv):
    """Every fragment's vector as the decoder derives it (thip_frontend.cpp, 7.5): (vx, vy) arrays [nfrags]."""
    vx, vy = np.zeros(geo.nfrags, np.int64), np.zeros(geo.nfrags, np.int64)
    for p, g in enumerate(geo.planes):
        nh = g["nhfrags"]
        loc = np.arange(g["nfrags"])
        fi = g["froffset"] + loc
        fy, fx = loc // nh, loc % nh
        mb = geo.mb_of[fi]
        x, y = mv[mb, 0].copy(), mv[mb, 1].copy()
        four = pix[mb] == MV_FOUR
        lx, ly = bmv[mb, :, 0], bmv[mb, :, 1]
        if p == 0:
            k = 2 * (fy & 1) + (fx & 1)
            x[four], y[four] = lx[four, k[four]], ly[four, k[four]]
        elif geo.hdec and geo.vdec:   # 4:2:0: the average of the four
            x[four], y[four] = round_div(lx[four].sum(1), 2), round_div(ly[four].sum(1), 2)
        elif geo.hdec:                # 4:2:2: the chroma block's row of two (bottom A, B; top C, D)
            a = 2 * (fy & 1)
            x[four] = round_div(lx[four, a[four]] + lx[four, a[four] + 1], 1)
            y[four] = round_div(ly[four, a[four]] + ly[four, a[four] + 1], 1)
        else:                         # 4:4:4: the luma block's own
            k = 2 * (fy & 1) + (fx & 1)
            x[four], y[four] = lx[four, k[four]], ly[four, k[four]]
        vx[fi], vy[fi] = x, y
    return vx, vy


def dc_residuals(geo, lev, coded, cls, nclasses, trace=None):
    """Spec 7.8 with reference classes 1..nclasses: dcr [nfrags] (the coded fragments' DC residuals).  trace (a list): gains
    (fragment, class, neighbour mask, which of the three 128-range corrections of mask 7 / 15 applied, else 0) per coded fragment."""
    dcr = np.zeros(geo.nfrags, np.int64)
    tdiv = lambda a, b: int(a / b) if a >= 0 else -int(-a / b)   # C division towards zero
    for p, g in enumerate(geo.planes):
        nh, o = g["nhfrags"], g["froffset"]
        last = {c: 0 for c in range(1, nclasses + 1)}
        for loc in range(g["nfrags"]):
            f = o + loc
            if not coded[f]:
                continue
            c = cls[f]
            fy, fx = loc // nh, loc % nh
            same = lambda q: coded[q] and cls[q] == c
            m, l, ul, u, ur, fix = 0, 0, 0, 0, 0, 0
            if fx > 0 and same(f - 1):
                m, l = m | 1, lev[f - 1, 0]
            if fy > 0:
                if fx > 0 and same(f - nh - 1):
                    m, ul = m | 2, lev[f - nh - 1, 0]
                if same(f - nh):
                    m, u = m | 4, lev[f - nh, 0]
                if fx + 1 < nh and same(f - nh + 1):
                    m, ur = m | 8, lev[f - nh + 1, 0]
            if m == 0:
                pred = last[c]
            elif m in (1, 3):
                pred = l
            elif m == 2:
                pred = ul
            elif m in (4, 6, 12):
                pred = u
            elif m == 5:
                pred = tdiv(l + u, 2)
            elif m == 8:
                pred = ur
            elif m in (9, 11, 13):
                pred = tdiv(75 * l + 53 * ur, 128)
            elif m == 10:
                pred = tdiv(ul + ur, 2)
            elif m == 14:
                pred = tdiv(3 * (ul + ur) + 10 * u, 16)
            else:
                pred = tdiv(29 * (l + u) - 26 * ul, 32)
                if abs(pred - u) > 128:
                    pred, fix = u, 1
                elif abs(pred - l) > 128:
                    pred, fix = l, 2
                elif abs(pred - ul) > 128:
                    pred, fix = ul, 3
            if trace is not None:
                trace.append((f, int(c), m, fix))
            dcr[f] = lev[f, 0] - pred
            last[c] = int(lev[f, 0])
    return dcr


class ModesEncoder(IR.InterEncoder):
    """The stream th_encode_* makes with TH_ENCCTL_THIP_SET_INTER_FRAMES and TH_ENCCTL_THIP_SET_INTER_MODES on.  frame() returns
    enc_inter_ref's dict plus modes8 (TH_ENCCTL_THIP_GET_MODE_STATS's modes) and vectors."""

    def frame(self, planes, qi, dups=0):
        out = super().frame(planes, qi, dups)
        if out["key"]:
            out.update(modes8=[0, len(self.geo.mb_order)] + [0] * 6, vectors=0)
        elif not out["packet"]:
            out.update(modes8=[0] * 8, vectors=0)
        return out

    def _inter(self, planes, qi):
        geo, setup = self.geo, self.setup
        src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]
        prev = [self.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
        gold = [self.ost.get_plane(oracle.FRAME_GOLD, p) for p in range(3)]
        tabs = {(qti, p): setup.qmat(qti, p, qi)[ZIGZAG] for qti in range(2) for p in range(3)}
        lam = int(tabs[(1, 0)][1])
        ms = motion_search(src[0], prev[0], gold[0], lam)
        pix, mv, bmv = ms["pix"], ms["mv"], ms["bmv"]
        fvx, fvy = fragment_vectors(geo, pix, mv, bmv)
        fpix = pix[geo.mb_of]
        fgold = (fpix == GOLDEN_NOMV) | (fpix == GOLDEN_MV)
        # blocks: prediction, residual, transform, quantiser (raster order)
        from tests import inter_stage_ref   # (it imports this module)
        lev, qti_of = inter_stage_ref.levels_of(geo, src, prev, gold, fpix, fvx, fvy, tabs)
        cls = np.where(qti_of == 0, 1, np.where(fgold, 3, 2))
        coded = (fpix != NOMV) | (lev != 0).any(1)
        ncoded = [int(coded[geo.froff[p]:geo.froff[p] + g["nfrags"]].sum()) for p, g in enumerate(geo.planes)]
        if not any(ncoded):
            return dict(packet=b"", modes=[0] * 5, coded=[0, 0, 0], mode_scheme=-1, mv_scheme=-1)
        dcr = dc_residuals(geo, lev, coded, cls, 3)
        bw = BitWriter()
        bw.write(0, 1)
        bw.write(1, 1)
        bw.write(qi, 6)
        bw.write(0, 1)
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
        costs = [mode_bits(freq, s, rank0) for s in range(8)]
        scheme = int(np.argmin(costs))
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
        # 7.7 tokens of the coded blocks
        cf = geo.coded_order[coded[geo.coded_order]]
        vals = lev[cf].copy()
        vals[:, 0] = dcr[cf]
        hti, ntok, nmerged, last_zzi = token_packet_tail(bw, vals, geo.plane_of[cf], setup)
        # the reconstruction: the oracle decodes the frame from the same lists, modes and vectors
        dq = np.stack([tabs[(int(qti_of[f]), int(geo.plane_of[f]))] for f in cf])
        coeffs = np.zeros((len(cf), 64), np.int64)
        coeffs[:, ZIGZAG] = lev[cf] * dq
        coeffs[:, 0] = lev[cf, 0]
        ost = self.ost
        ost.coded[:] = coded
        refi = np.array([MODE_REFI[int(m)] for m in mb_mode[geo.mb_of]], np.uint8)
        refi[~coded] = 3
        ost.refi[:] = refi
        ost.mvs[:] = ((fvx & 0xFF) | (fvy << 8)).astype(np.int16)
        unc = geo.coded_order[~coded[geo.coded_order]]
        ost.decode_frame(frame_type=1, coded_fragis=cf, ncoded=ncoded, coeffs=coeffs.astype(np.int16), last_zzi=last_zzi,
                         dc_quant=dq[:, 0].astype(np.uint16), uncoded_fragis=unc, flimit=setup.lflims[qi])
        return dict(packet=bw.bytes(), modes=counts[:5], modes8=counts, vectors=len(mvs), coded=ncoded, mode_scheme=scheme,
                    mv_scheme=mvmode, huff=hti, tokens=ntok, tokens_merged=nmerged, coded_fragis=cf, pix=pix, search=ms)


class RateStream(enc_rate_ref.RateStream):
    """enc_rate_ref's bitrate-mode stream with the eight-mode encoder: the probe and the controller are unchanged (the probe still
    models five modes), the frames are coded at the chosen qi with the eight-mode search."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, fps=(30, 1), inter=False, kf_interval=64, shift=6, **kw):
        super().__init__(fw, fh, fmt, pic, setup, bitrate, fps=fps, inter=inter, kf_interval=kf_interval, shift=shift, **kw)
        self.enc.close()
        self.enc = ModesEncoder(fw, fh, fmt, pic, setup, kf_interval if inter else 1, shift)


# ---- content ------------------------------------------------------------------------------------------------------------------
def _textured(h, w, seed, luma):
    """A natural image; in luma, half of it fine noise (texture that no neighbouring position predicts)."""
    a = enc_ref.content("natural", (h, w), seed).astype(np.int64)
    if luma:
        a = (a + enc_ref.content("noise", (h, w), seed + 101)) >> 1
    return a.astype(np.uint8)


def sequence(kind, fw, fh, fmt, nframes, seed=0):
    """Frames (three top-first planes each) of frame size fw x fh: enc_inter_ref.sequence's kinds, and
      uncover  a still, textured background; from the second frame a textured object (three quarters of the frame high, half as wide) crosses it from
               left to right, twelve pixels a frame, and from the middle of the clip on it has left, uncovering what the first frame (a
               key frame) showed
      shear    horizontal bands 8 luma rows high over a textured image, moving in opposite directions, four pixels a frame"""
    if kind not in ("uncover", "shear"):
        return IR.sequence(kind, fw, fh, fmt, nframes, seed)
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    out = []
    if kind == "uncover":
        bg = [_textured(fh + 32, fw + 32, seed + p, p == 0) for p in range(3)]
        ob = [enc_ref.content("natural", (fh + 32, fw + 32), seed + 11 + p) for p in range(3)]
        oh, ow = max(3 * fh // 4, 8) & ~1, max(fw // 2, 8) & ~1
        oy = (fh // 8) & ~1
        for f in range(nframes):
            # the object's left edge: off the picture in the first frame, then 0, 12, 24, ...; from frame (n + 1) / 2 on it has left
            ox = -ow if f == 0 or f >= (nframes + 1) // 2 else 12 * (f - 1)
            fr = []
            for p in range(3):
                sx, sy = (hd, vd) if p else (0, 0)
                a = bg[p][16:16 + fh, 16:16 + fw][::1 + sy, ::1 + sx].copy()
                y0, y1 = oy >> sy, (oy + oh) >> sy
                x0, x1 = max(ox, 0) >> sx, max(min(ox + ow, fw), 0) >> sx
                if x1 > x0:
                    # the object's texture moves with it (a window of its own image at its position)
                    a[y0:y1, x0:x1] = ob[p][16 + y0:16 + y1, 16 + x0 - (ox >> sx):16 + x1 - (ox >> sx)]
                fr.append(np.ascontiguousarray(a))
            out.append(fr)
        return out
    big = [_textured(fh + 8, fw + 8 * nframes + 16, seed + p, p == 0) for p in range(3)]
    for f in range(nframes):
        fr = []
        for p in range(3):
            sx, sy = (hd, vd) if p else (0, 0)
            a = np.empty((fh >> sy, fw >> sx), np.uint8)
            bh = 8 >> sy
            for b in range(0, fh // 8):
                x = 4 * nframes + 8 + (4 * f if b % 2 == 0 else -4 * f)
                a[b * bh:(b + 1) * bh] = big[p][b * 8 + 4:b * 8 + 12:1 + sy, x:x + fw:1 + sx][:bh, :fw >> sx]
            fr.append(a)
        out.append(fr)
    return out
