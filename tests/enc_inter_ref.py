"""enc_inter_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s inter frames (include/theoraenc_hip.h, "Inter frames") in
numpy, to compare the library's packets with byte for byte.

Key frames are tests/enc_ref.py's.  The reference of an inter frame is the oracle's decode of the packets restated so far (its
PREV frame), so the restatement also states the reconstruction the encoder must reach.  The syntax writers are streamgen's
(write_long_runs, write_short_runs, write_mv, MODE_ALPHABETS); the transform and quantiser are the oracle's.
"""
import numpy as np

import oracle
from tests import enc_ref
from tests.enc_ref import ZIGZAG, block_tokens, huff_group
from tests.streamgen import MODE_ALPHABETS, BitWriter, eob_token, write_long_runs, write_mv, write_short_runs

NOMV, INTRA, MV, MV_LAST, MV_LAST2 = range(5)
MODE_REFI = {NOMV: 1, INTRA: 2, MV: 1, MV_LAST: 1, MV_LAST2: 1}   # oracle reference index: PREV 1, SELF 2


def mv_axis(v, quarter):
    """The decoder's offsets of one vector component (thip_device.h mv_axis, spec 7.9.4): whole part towards zero, second read's step."""
    v = np.asarray(v, np.int64)
    sh = 2 if quarter else 1
    m = (1 << sh) - 1
    whole = (v + ((v >> 63) & m)) >> sh
    frac = np.where(v & m, np.where(v < 0, -1, 1), 0)
    return whole, frac


def predict(ref, x, y, mvx, mvy, qpx, qpy):
    """Predictor pixels at integer arrays (x, y) (bitstream rows) of plane `ref` (bitstream order) for vectors (mvx, mvy)."""
    H, W = ref.shape
    mx, mx2 = mv_axis(mvx, qpx)
    my, my2 = mv_axis(mvy, qpy)
    a = ref[np.clip(y + my, 0, H - 1), np.clip(x + mx, 0, W - 1)].astype(np.int64)
    b = ref[np.clip(y + my + my2, 0, H - 1), np.clip(x + mx + mx2, 0, W - 1)].astype(np.int64)
    return (a + b) >> 1


def search_stats(src, ref):
    """Luma search of every macro block (raster, rows from the bottom), what of it does not depend on lambda: (mvx, mvy, S0, SI,
    Smv) arrays, the vector the half-pel one found."""
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
        p = predict(ref, X, Y, mvx[:, None, None], mvy[:, None, None], False, False)
        sad = np.abs(sblk - p).sum((1, 2))
        cur = np.minimum(cur, (sad << 32) | ((np.abs(mvx) + np.abs(mvy)) << 16) | k9)
    k9 = cur & 0xFFFF
    mvx, mvy = 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1
    smv = cur >> 32
    b4 = sblk.reshape(-1, 2, 8, 2, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 4, 64)
    mean = (b4.sum(2) + 32) >> 6
    si = np.abs(b4 - mean[:, :, None]).sum((1, 2))
    return mvx, mvy, s0, si, smv


def decide(stats, lam):
    """The five-mode rule over search_stats' arrays: (pixel mode, mvx, mvy, S0, SI, Smv), the vector zero unless MV."""
    mvx, mvy, s0, si, smv = stats
    mode = np.where(smv + lam < s0, MV, NOMV)
    sinter = np.where(mode == MV, smv, s0)
    mode = np.where(si + 4 * lam < sinter, INTRA, mode)
    mvx = np.where(mode == MV, mvx, 0)
    mvy = np.where(mode == MV, mvy, 0)
    return mode, mvx, mvy, s0, si, smv


def motion_search(src, ref, lam):
    """Luma search of every macro block (raster, rows from the bottom): (pixel mode, mvx, mvy, S0, SI, Smv) arrays."""
    return decide(search_stats(src, ref), lam)


class Geometry:
    def __init__(self, fw, fh, fmt):
        st = oracle.State(fw, fh, fmt)
        self.planes = [dict(st.planes[p]) for p in range(3)]
        self.coded_order = np.concatenate([st.sb_order(p) for p in range(3)])
        st.close()
        self.hdec, self.vdec = int(not (fmt & 1)), int(not (fmt & 2))
        self.froff = [g["froffset"] for g in self.planes]
        self.nfrags = sum(g["nfrags"] for g in self.planes)
        self.plane_of = np.concatenate([np.full(g["nfrags"], p) for p, g in enumerate(self.planes)])
        self.sb_len = []
        for g in self.planes:
            nh, nv = g["nhfrags"], g["nvfrags"]
            for sy in range(0, nv, 4):
                for sx in range(0, nh, 4):
                    self.sb_len.append(min(4, nv - sy) * min(4, nh - sx))
        nh, nv = self.planes[0]["nhfrags"], self.planes[0]["nvfrags"]
        self.nmbx = nh // 2
        self.mb_order = []
        for sy in range(0, nv, 4):
            for sx in range(0, nh, 4):
                for my, mx in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    y, x = sy + 2 * my, sx + 2 * mx
                    if y < nv and x < nh:
                        self.mb_order.append((y >> 1) * self.nmbx + (x >> 1))
        # every fragment's macro block (raster)
        self.mb_of = np.empty(self.nfrags, np.int64)
        for p, g in enumerate(self.planes):
            loc = np.arange(g["nfrags"])
            fy, fx = loc // g["nhfrags"], loc % g["nhfrags"]
            sx, sy = (1 - self.hdec, 1 - self.vdec) if p else (1, 1)
            self.mb_of[g["froffset"] + loc] = (fy >> sy) * self.nmbx + (fx >> sx)


def token_packet_tail(bw, vals_by_block, plane_of, setup, detail=None):
    """Tokens of the coded blocks (zig-zag values, DC the residual; coded order) appended to bw as enc_ref.encode_frame writes them:
    EOB runs merged across lists and planes, the tables of least bits.  Returns (hti, ntok, nmerged, last_zzi).  detail: a dict that
    receives words (the tokens before the merge in stream order, in the word format of thip_encode.h) and list_len [64][3], as
    enc_ref.encode_frame hands them out."""
    by_z, last_zzi = {}, []
    for v, p in zip(vals_by_block, plane_of):
        toks = block_tokens(v)
        last_zzi.append(toks[-1][0])
        for t in toks:
            by_z.setdefault((t[0], int(p)), []).append(t[1:])
    ntok = sum(len(v) for v in by_z.values())
    if detail is not None:
        detail["words"] = np.array([(z << 16 | p << 22) | (0 if t[0] == "EOB" else t[0] | t[1] << 5)
                                    for z in range(64) for p in range(3) for t in by_z.get((z, p), [])], np.uint32)
        detail["list_len"] = np.array([[len(by_z.get((z, p), [])) for p in range(3)] for z in range(64)], np.int64)
    lists, run, rstart = {}, 0, None

    def flush():
        nonlocal run
        if run:
            lists.setdefault(rstart, []).append(eob_token(run))
            run = 0
    for z in range(64):
        for p in range(3):
            for t in by_z.get((z, p), []):
                if t[0] == "EOB":
                    if run == 0:
                        rstart = (z, p)
                    run += 1
                    if run == 4095:
                        flush()
                    continue
                flush()
                lists.setdefault((z, p), []).append(t)
    flush()
    hist = np.zeros((5, 2, 32), np.int64)
    for (z, p), toks in lists.items():
        for t in toks:
            hist[huff_group(z), int(p > 0), t[0]] += 1
    lens = np.array([[len(setup.codes[h].get(t, "")) for t in range(32)] for h in range(80)], np.int64)
    hti = []
    for c in range(4):
        ac, ch = c >> 1, c & 1
        groups = range(1, 5) if ac else range(0, 1)
        cost = [sum(int(hist[hg, ch] @ lens[16 * hg + t]) for hg in groups) for t in range(16)]
        hti.append(int(np.argmin(cost)))
    for z in range(64):
        if z < 2:
            bw.write(hti[2 * z], 4)
            bw.write(hti[2 * z + 1], 4)
        for p in range(3):
            codes = setup.codes[16 * huff_group(z) + hti[(2 if z else 0) + int(p > 0)]]
            for tok, extra, nb in lists.get((z, p), []):
                bw.code(codes[tok])
                bw.write(extra, nb)
    return hti, ntok, sum(len(v) for v in lists.values()), np.asarray(last_zzi, np.uint8)


def mode_bits(freq, scheme, rank0):
    if scheme == 7:
        return 3 * sum(freq)
    rank = rank0 if scheme == 0 else [MODE_ALPHABETS[scheme - 1].index(m) for m in range(8)]
    return (24 if scheme == 0 else 0) + sum(f * (rank[m] + 1 if rank[m] < 7 else 7) for m, f in enumerate(freq))


def mv_vlc_bits(v):
    a = abs(v)
    return 3 if a <= 1 else 4 if a <= 3 else 6 if a <= 7 else 7 if a <= 15 else 8


class InterEncoder:
    """The stream th_encode_* makes with TH_ENCCTL_THIP_SET_INTER_FRAMES on.  frame(planes, qi, dups) -> dict(packet, key, ...);
    self.recon: the reconstruction (three planes, rows top first) after the last frame."""

    def __init__(self, fw, fh, fmt, pic, setup, kf_interval, shift):
        self.fw, self.fh, self.fmt, self.pic, self.setup = fw, fh, fmt, pic, setup
        self.kf_interval, self.shift = kf_interval, shift
        self.geo = Geometry(fw, fh, fmt)
        self.ost = oracle.State(fw, fh, fmt)
        self.cur, self.key = -1, -1

    def close(self):
        self.ost.close()

    @property
    def recon(self):
        return [self.ost.get_plane(oracle.FRAME_PREV, p)[::-1].copy() for p in range(3)]

    def frame(self, planes, qi, dups=0):
        f = self.cur + 1
        off = f - self.key
        key = self.key < 0 or off >= self.kf_interval or off + dups >= (1 << self.shift)
        out = self._key(planes, qi) if key else self._inter(planes, qi)
        if key:
            self.key = f
        self.cur = f + dups
        out["key"] = key
        return out

    def _key(self, planes, qi):
        ref = enc_ref.encode_frame(planes, self.fw, self.fh, self.fmt, self.pic, qi, self.setup)
        enc_ref.oracle_decode(self.ost, ref)
        nmbs = len(self.geo.mb_order)
        return dict(packet=ref["packet"], modes=[0, nmbs, 0, 0, 0], coded=[g["nfrags"] for g in self.geo.planes],
                    mode_scheme=-1, mv_scheme=-1)

    def _inter(self, planes, qi):
        geo, setup = self.geo, self.setup
        src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]
        ref = [self.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
        tabs = {(qti, p): setup.qmat(qti, p, qi)[ZIGZAG] for qti in range(2) for p in range(3)}
        lam = int(tabs[(1, 0)][1])
        pix, mvx, mvy = motion_search(src[0], ref[0], lam)[:3]
        # blocks: prediction, residual, transform, quantiser (raster order)
        from tests import inter_stage_ref   # (it imports this module)
        lev, qti_of = inter_stage_ref.levels_of(geo, src, ref, None, pix[geo.mb_of], mvx[geo.mb_of], mvy[geo.mb_of], tabs)
        cls = np.where(qti_of == 0, 1, 2)
        coded = (pix[geo.mb_of] != NOMV) | (lev != 0).any(1)
        ncoded = [int(coded[geo.froff[p]:geo.froff[p] + g["nfrags"]].sum()) for p, g in enumerate(geo.planes)]
        if not any(ncoded):
            return dict(packet=b"", modes=[0] * 5, coded=[0, 0, 0], mode_scheme=-1, mv_scheme=-1)
        # DC residuals: spec 7.8 with reference classes, the last coded DC of the class in raster order as the fallback
        dcr = np.zeros(geo.nfrags, np.int64)
        tdiv = lambda a, b: int(a / b) if a >= 0 else -int(-a / b)   # C division towards zero
        for p, g in enumerate(geo.planes):
            nh, o = g["nhfrags"], g["froffset"]
            last = {1: 0, 2: 0}
            for loc in range(g["nfrags"]):
                f = o + loc
                if not coded[f]:
                    continue
                c = cls[f]
                fy, fx = loc // nh, loc % nh
                same = lambda q: coded[q] and cls[q] == c
                m, l, ul, u, ur = 0, 0, 0, 0, 0
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
                        pred = u
                    elif abs(pred - l) > 128:
                        pred = l
                    elif abs(pred - ul) > 128:
                        pred = ul
                dcr[f] = lev[f, 0] - pred
                last[c] = int(lev[f, 0])
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
        counts = [0] * 5
        mb_mode = np.full(len(pix), NOMV)
        for mb in geo.mb_order:
            f0 = 2 * (mb // geo.nmbx) * nh0 + 2 * (mb % geo.nmbx)
            if not (coded[f0] or coded[f0 + 1] or coded[f0 + nh0] or coded[f0 + nh0 + 1]):
                counts[NOMV] += 1
                continue
            mode = int(pix[mb])
            if mode == MV:
                v = (int(mvx[mb]), int(mvy[mb]))
                if v == last1:
                    mode = MV_LAST
                elif v == last2:
                    mode = MV_LAST2
                    last2, last1 = last1, v
                else:
                    mvs.append(v)
                    last2, last1 = last1, v
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
        detail = {}
        hti, ntok, nmerged, last_zzi = token_packet_tail(bw, vals, geo.plane_of[cf], setup, detail)
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
        vx, vy = mvx[geo.mb_of], mvy[geo.mb_of]
        ost.mvs[:] = ((vx & 0xFF) | (vy << 8)).astype(np.int16)
        unc = geo.coded_order[~coded[geo.coded_order]]
        ost.decode_frame(frame_type=1, coded_fragis=cf, ncoded=ncoded, coeffs=coeffs.astype(np.int16), last_zzi=last_zzi,
                         dc_quant=dq[:, 0].astype(np.uint16), uncoded_fragis=unc, flimit=setup.lflims[qi])
        return dict(packet=bw.bytes(), modes=counts, coded=ncoded, mode_scheme=scheme, mv_scheme=mvmode, huff=hti, tokens=ntok,
                    tokens_merged=nmerged, coded_fragis=cf, mvx=mvx, mvy=mvy, pix=pix, levels=lev[geo.coded_order], dcr=dcr,
                    cmap=np.where(coded, cls, 0).astype(np.uint8), words=detail["words"], list_len=detail["list_len"])


# ---- content ------------------------------------------------------------------------------------------------------------------
def sequence(kind, fw, fh, fmt, nframes, seed=0):
    """Frames (three top-first planes each) of a moving test sequence of frame size fw x fh:
      pan      a crop window over a larger natural image, moving by whole and by odd half-pixel-scale offsets
      static   the same picture repeated (uncoded blocks)
      cut      a pan that cuts to noise half way (INTRA macro blocks)"""
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    big = [enc_ref.content("natural", (fh + 96, fw + 96), seed + p) for p in range(3)]
    steps = [(0, 0), (3, 1), (4, -2), (1, 5), (-3, 3), (0, 0), (7, -1), (-5, -6), (2, 2), (9, 4)]
    out, x, y = [], 40, 40
    for f in range(nframes):
        if kind == "static":
            dx, dy = 0, 0
        else:
            dx, dy = steps[f % len(steps)]
        x, y = int(np.clip(x + dx, 0, 80)), int(np.clip(y + dy, 0, 80))
        if kind == "cut" and f >= nframes // 2:
            out.append([enc_ref.content("noise", s, seed + 7 * f + p) for p, s in
                        enumerate([(fh, fw), (fh >> vd, fw >> hd), (fh >> vd, fw >> hd)])])
            continue
        fr = [big[0][y:y + fh, x:x + fw]]
        for p in (1, 2):
            # chroma: the luma window, subsampled by picking (keeps whole-pixel motion whole in luma)
            fr.append(big[p][y:y + fh:1 + vd, x:x + fw:1 + hd].copy())
        out.append([np.ascontiguousarray(a) for a in fr])
    return out
