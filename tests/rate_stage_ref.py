"""rate_stage_ref.py -- TEST INFRASTRUCTURE: the rate probe of th_encode_*'s bitrate mode (theora_amd/csrc/thip_rate.h), one function
per stage, with the shapes thip_enc_rate_stage (include/theora_hip.h) hands its results out in.  The transform and the quantiser are the
oracle's, the prediction and the mode rule enc_inter_ref's; the token counting is a vectorised statement of enc_ref.block_tokens with
every EOB its own token (tests/test_rate_stage_cpu.py holds it against that scalar loop), the DC prediction a masked statement of
spec 7.8 (held against enc_ref.dc_predict and a scalar one there).  tests/enc_rate_ref.py's Probe is a composition of these functions.

Everything is in bitstream coordinates: fragments in raster order from the bottom row, plane after plane.
  coef     int16 [1 or 3][n][64], NATURAL order: the transform of each block's residual -- inter: INTRA (pixel - 128), NOMV, MV
  steps    uint16 [6][64 q][64 z], zig-zag: table 0..2 intra, 3..5 inter of each plane
  stats    k_rate_me's words, uint32 [nmbs][4]: S0, Smv, SI, mvx & 0xFF | (mvy & 0xFF) << 8
  qdc      int16 [n][64 q];  coded, cls  uint64 [n], bit q
  partial  int64 [groups][64 q][321]: counts [luma / chroma][Huffman group][token], then the side count
"""
import numpy as np

import oracle
from tests import enc_ref
from tests import enc_inter_ref as IR
from tests.enc_ref import ZIGZAG
from tests.enc_inter_ref import INTRA, MV, NOMV

EXTRA_BITS = np.array([0, 0, 0, 2, 3, 4, 12, 3, 6, 0, 0, 0, 0, 1, 1, 1, 1, 2, 3, 4, 5, 6, 10, 1, 1, 1, 1, 1, 3, 4, 2, 3], np.int64)
HG = np.array([enc_ref.huff_group(z) for z in range(65)], np.int64)   # (index 64: never used)
BINS, WAVES = 320, 16
FIXED_KEY = 28   # header bits: 0, frame type, qi, 0, 3 reserved bits, the four table indices


def fixed_inter(n):
    return 25 + n // 8


def geometry(fw, fh, fmt):
    return IR.Geometry(fw, fh, fmt)


# ---- tables --------------------------------------------------------------------------------------------------------------------
def steps_of(setup):
    """The steps of a setup header (enc_ref.SetupParams)."""
    return np.array([[setup.qmat(t // 3, t % 3, q)[ZIGZAG] for q in range(64)] for t in range(6)], np.uint16)


def steps_flat(step=1):
    return np.full((6, 64, 64), step, np.uint16)


def steps_decreasing(base=3, scale=3):
    """Strictly decreasing in q at every index, every table its own: base + table + (z & 3) + scale * (63 - q), so every q quantises
    differently and qi 63 holds the least step.  (An odd scale: a step's parity alternates with q and with the table, and only an even
    step d has a coefficient with 2|c| = d.)"""
    t, q, z = np.ogrid[0:6, 0:64, 0:64]
    return (base + t + (z & 3) + scale * (63 - q)).astype(np.uint16)


def code_lengths(setup):
    return np.array([[len(setup.codes[h].get(t, "")) for t in range(32)] for h in range(80)], np.int64)


def to_natural(zz):
    out = np.empty_like(zz)
    out[..., ZIGZAG] = zz
    return out


# ---- COEF ----------------------------------------------------------------------------------------------------------------------
def _plane_xy(geo, p):
    g = geo.planes[p]
    nh = g["nhfrags"]
    loc = np.arange(g["nfrags"])
    fy, fx = loc // nh, loc % nh
    r = np.arange(8)
    return fy[:, None, None] * 8 + r[None, :, None], fx[:, None, None] * 8 + r[None, None, :]


def _fdct(res):
    return to_natural(oracle.fdct8x8_batch(res.reshape(-1, 64).astype(np.int16)))


def coef_key(geo, src):
    """src: the three frame-sized planes the encoder transforms (inter_stage_ref.frame_src).  -> [1][n][64]"""
    out = []
    for p in range(3):
        Y, X = _plane_xy(geo, p)
        out.append(_fdct(src[p][Y, X] - 128))
    return np.concatenate(out)[None]


def coef_inter(geo, src, prev, mvx, mvy):
    """prev: the reference's three planes; mvx, mvy [nmbs]: the half-pel vector of every macro block (stats' own).  -> [3][n][64]"""
    out = [[], [], []]
    for p, g in enumerate(geo.planes):
        Y, X = _plane_xy(geo, p)
        mb = geo.mb_of[g["froffset"] + np.arange(g["nfrags"])]
        qx, qy = p > 0 and geo.hdec, p > 0 and geo.vdec
        pix = src[p][Y, X]
        zero = np.zeros(len(mb), np.int64)[:, None, None]
        for v, pred in enumerate((128, IR.predict(prev[p], X, Y, zero, zero, qx, qy),
                                  IR.predict(prev[p], X, Y, mvx[mb][:, None, None], mvy[mb][:, None, None], qx, qy))):
            out[v].append(_fdct(pix - pred))
    return np.stack([np.concatenate(o) for o in out])


def pack_stats(s0, smv, si, mvx, mvy):
    b = lambda v: np.asarray(v, np.int64) & 0xFF
    return np.stack([s0, smv, si, b(mvx) | b(mvy) << 8], 1).astype(np.uint32)


def stats_vectors(stats):
    w = np.asarray(stats, np.int64)[:, 3]
    sx = lambda v: ((v & 0xFF) ^ 0x80) - 0x80
    return sx(w), sx(w >> 8)


# ---- the levels at one q -------------------------------------------------------------------------------------------------------
def modes_at(stats, lam):
    """rate_mode: the mode of every macro block from its word and lambda (enc_inter_ref.decide's rule)."""
    s = np.asarray(stats, np.int64).astype(np.int32).astype(np.int64)   # (the kernel reads the words as int)
    return IR.decide((0, 0, s[:, 0], s[:, 2], s[:, 1]), int(lam))[0]


def _frag_modes(geo, inter, stats, lam, q):
    if not inter:
        return np.full(geo.nfrags, INTRA)
    return modes_at(stats, lam[q])[geo.mb_of]


_VAR = {INTRA: 0, NOMV: 1, MV: 2}


def levels_at(geo, coef, steps, q, fmode):
    """[n][64] zig-zag levels of every block at q: the residual and the table of its mode fmode [n]."""
    coef = np.asarray(coef)
    lev = np.zeros((geo.nfrags, 64), np.int64)
    for p, g in enumerate(geo.planes):
        fi = g["froffset"] + np.arange(g["nfrags"])
        for m, v in _VAR.items():
            sel = fi[fmode[fi] == m]
            if len(sel):
                lev[sel] = oracle.quantize_batch(coef[v if coef.shape[0] == 3 else 0][sel][:, ZIGZAG], steps[(0 if m == INTRA else 3) + p, q])[0]
    return lev


def _bits(mask_by_q):
    """bool [n][64] -> uint64 [n]"""
    return (mask_by_q.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)


def bit(words, q):
    return ((np.asarray(words, np.uint64) >> np.uint64(q)) & np.uint64(1)).astype(bool)


# ---- DC ------------------------------------------------------------------------------------------------------------------------
def dc_stage(geo, coef, steps, inter, stats=None, lam=None, keep=None):
    """-> qdc [n][64], coded, cls uint64 [n] (a key frame: every block coded at every q, class 0).  keep: a dict that receives the
    levels of each q, for a tok_stage over the same coefficients, tables and modes."""
    n = geo.nfrags
    qdc = np.zeros((n, 64), np.int16)
    coded = np.ones((n, 64), bool)
    cls = np.zeros((n, 64), bool)
    for q in range(64):
        fmode = _frag_modes(geo, inter, stats, lam, q)
        lev = levels_at(geo, coef, steps, q, fmode)
        if keep is not None:
            keep[q] = lev
        qdc[:, q] = lev[:, 0]
        if inter:
            coded[:, q] = (fmode != NOMV) | (lev != 0).any(1)
            cls[:, q] = fmode != INTRA
    return qdc, _bits(coded), _bits(cls)


# ---- DC prediction -------------------------------------------------------------------------------------------------------------
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
    m = neighbour_mask(avail)
    l, ul, u, ur = (np.where(avail[..., k], v, 0) for k, v in enumerate((l, ul, u, ur)))
    p15 = _tdiv(29 * (l + u) - 26 * ul, 32)
    p15 = np.where(np.abs(p15 - u) > 128, u, np.where(np.abs(p15 - l) > 128, l, np.where(np.abs(p15 - ul) > 128, ul, p15)))
    return np.select([np.isin(m, (1, 3)), m == 2, np.isin(m, (4, 6, 12)), m == 5, m == 8, np.isin(m, (9, 11, 13)), m == 10, m == 14,
                      np.isin(m, (7, 15))],
                     [l, ul, u, _tdiv(l + u, 2), ur, _tdiv(75 * l + 53 * ur, 128), _tdiv(ul + ur, 2), _tdiv(3 * (ul + ur) + 10 * u, 16),
                      p15], 0)


def neighbour_mask(avail):
    return avail[..., 0] * 1 + avail[..., 1] * 2 + avail[..., 2] * 4 + avail[..., 3] * 8


def neighbour_avail(ok, same):
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


def dc_residuals(geo, dc, ok, cl):
    """The DC residual of every fragment (raster) from the quantised DCs dc [n], the coded flags ok and the classes cl; and the
    neighbour mask each was predicted with."""
    res, msk = np.zeros(geo.nfrags, np.int64), np.zeros(geo.nfrags, np.int64)
    for g in geo.planes:
        nv, nh = g["nvfrags"], g["nhfrags"]
        s = slice(g["froffset"], g["froffset"] + g["nfrags"])
        avail = neighbour_avail(ok[s].reshape(nv, nh), cl[s].reshape(nv, nh))
        d = dc[s].astype(np.int64).reshape(nv, nh)
        res[s] = (d - dc_pred_masked(d, avail)).reshape(-1)
        msk[s] = neighbour_mask(avail).reshape(-1)
    return res, msk


# ---- TOK -----------------------------------------------------------------------------------------------------------------------
def _value_token(a):
    """enc_ref's smallest value token of non-zero levels a (array)."""
    aa, s = np.abs(a), (a < 0).astype(np.int64)
    return np.select([aa == 1, aa == 2, aa <= 6, aa <= 8, aa <= 12, aa <= 20, aa <= 36, aa <= 68],
                     [9 + s, 11 + s, 10 + aa, 17, 18, 19, 20, 21], 22)


def token_hist(vals, chroma, part=None, nparts=None):
    """Tokens of blocks vals [N, 64] (zig-zag, DC the residual), each EOB its own token: counts [2][5][32] by (chroma, Huffman group
    of the start index, token) -- enc_ref.block_tokens, vectorised.  With part [N] (each block's partial) and nparts: [nparts][2][5][32]."""
    split = part is not None
    hist = np.zeros((nparts if split else 1, 2, 5, 32), np.int64)
    n = len(vals)
    if n:
        part = np.asarray(part, np.int64) if split else np.zeros(n, np.int64)
        nz = vals != 0
        idx = np.arange(64)
        last = np.where(nz, idx, -1)
        prev = np.maximum.accumulate(np.concatenate([np.full((n, 1), -1), last[:, :-1]], 1), axis=1)   # last non-zero before z
        b, z = np.nonzero(nz)
        a, start = vals[b, z], prev[b, z] + 1
        gap = z - start
        cc = np.asarray(chroma)[b].astype(np.int64)
        pp = part[b]
        aa = np.abs(a)
        cat1 = (aa == 1) & (gap >= 1) & (gap <= 17)
        cat2 = ~cat1 & ((aa == 2) | (aa == 3)) & (gap >= 1) & (gap <= 3)
        plain = ~cat1 & ~cat2
        t1 = np.where(gap <= 5, 22 + gap, np.where(gap <= 9, 28, 29))
        t2 = np.where(gap == 1, 30, 31)
        np.add.at(hist, (pp[cat1], cc[cat1], HG[start[cat1]], t1[cat1]), 1)
        np.add.at(hist, (pp[cat2], cc[cat2], HG[start[cat2]], t2[cat2]), 1)
        zr = plain & (gap > 0)
        np.add.at(hist, (pp[zr], cc[zr], HG[start[zr]], np.where(gap[zr] <= 8, 7, 8)), 1)
        np.add.at(hist, (pp[plain], cc[plain], HG[z[plain]], _value_token(a[plain])), 1)
        end = last.max(1) + 1
        eob = end < 64
        np.add.at(hist, (part[eob], np.asarray(chroma)[eob].astype(np.int64), HG[end[eob]], 0), 1)
    return hist if split else hist[0]


def group_of(n, groups):
    """The work group that takes each block: wave w of group wg takes the blocks wg * 16 + w + k * 16 * groups."""
    return (np.arange(n) // WAVES) % groups


def tok_stage(geo, coef, qdc, coded, cls, steps, inter, stats=None, lam=None, groups=1, kept=None):
    """-> partial [groups][64][321].  A key frame reads neither coded nor cls.  The AC levels follow the block's mode at q (stats and
    lambda), the DC is qdc less its prediction among the neighbours coded at q in the block's class at q, as given."""
    n = geo.nfrags
    part = group_of(n, groups)
    chroma = np.arange(n) >= geo.planes[1]["froffset"]
    out = np.zeros((groups, 64, BINS + 1), np.int64)
    g0 = geo.planes[0]
    nh0, nv0 = g0["nhfrags"], g0["nvfrags"]
    first = (np.arange(nv0)[0::2, None] * nh0 + np.arange(nh0)[None, 0::2]).reshape(-1)   # each macro block's first luma block
    qdc = np.asarray(qdc)
    for q in range(64):
        fmode = _frag_modes(geo, inter, stats, lam, q)
        ok = bit(coded, q) if inter else np.ones(n, bool)
        cl = bit(cls, q) if inter else np.zeros(n, bool)
        vals = kept[q].copy() if kept else levels_at(geo, coef, steps, q, fmode)
        vals[:, 0] = dc_residuals(geo, qdc[:, q], ok, cl)[0]
        out[:, q, :BINS] = token_hist(vals[ok], chroma[ok], part[ok], groups).reshape(groups, BINS)
        if inter:
            # side bits: 3 a macro block with a coded luma block, 12 more when it is MV; counted where its first luma block is
            c0 = ok[:g0["nfrags"]].reshape(nv0, nh0)
            mbc = (c0[0::2, 0::2] | c0[0::2, 1::2] | c0[1::2, 0::2] | c0[1::2, 1::2]).reshape(-1)
            np.add.at(out[:, q, BINS], part[first], mbc * np.where(fmode[first] == MV, 15, 3))
    return out


# ---- BITS ----------------------------------------------------------------------------------------------------------------------
def table_costs(hist, lens):
    """[4 choices (DC luma, DC chroma, AC luma, AC chroma)][16 tables]: the bits of hist [2][5][32] under each table."""
    out = np.zeros((4, 16), np.int64)
    for c in range(4):
        ac, cc = c >> 1, c & 1
        for t in range(16):
            out[c, t] = sum(int(hist[cc, hg] @ lens[16 * hg + t]) for hg in (range(1, 5) if ac else range(0, 1)))
    return out


def hist_bits(hist, lens):
    """The least bits of each table choice (DC luma, DC chroma, AC luma, AC chroma) plus the extra bits."""
    return int((hist.sum((0, 1)) * EXTRA_BITS).sum()) + int(table_costs(hist, lens).min(1).sum())


def bits_stage(partial, lens, fixed):
    """-> E [64]"""
    tot = np.asarray(partial, np.int64).sum(0)
    lens = np.asarray(lens, np.int64).reshape(80, 32)
    return np.array([fixed + int(tot[q, BINS]) + hist_bits(tot[q, :BINS].reshape(2, 5, 32), lens) for q in range(64)], np.int64)


# ---- composed ------------------------------------------------------------------------------------------------------------------
def probe(geo, coef, steps, lens, inter, stats=None, lam=None, groups=1):
    kept = {}
    qdc, coded, cls = dc_stage(geo, coef, steps, inter, stats, lam, kept)
    fixed = fixed_inter(geo.nfrags) if inter else FIXED_KEY
    return bits_stage(tok_stage(geo, coef, qdc, coded, cls, steps, inter, stats, lam, groups, kept), lens, fixed)


# ---- planted content -----------------------------------------------------------------------------------------------------------
STARTS = (0, 1, 5, 6, 14, 15, 27, 28)   # a start index in every Huffman group, and the last of each group but the fifth
BOUNDARY_LEVELS = (2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 20, 21, 36, 37, 68, 69)   # either side of every value token's range (and 4, 5)


def edge_blocks():
    """The token edges as blocks of zig-zag values [N, 64] (index 0: the DC RESIDUAL), and what each is: (kind, start, gap, value).
    A token that starts at index s > 0 follows a 4 at s - 1.  Each start of STARTS gets: a gap of 0..6, 9, 10, 17, 18 before +-1;
    of 0..4 before +-2 and +-3; zero runs of 8, 9 and 62 before a 5; every boundary level of both signs at the start itself.  Then the
    block ends: the last value at index 62 and at 63, the empty block, the DC-only block."""
    blocks, what = [], []

    def add(kind, s, gap, v):
        if s + gap > 63:
            return
        b = np.zeros(64, np.int64)
        if s > 0:
            b[s - 1] = 4
        b[s + gap] = v
        blocks.append(b)
        what.append((kind, s, gap, v))
    for s in STARTS:
        for gap in (0, 1, 2, 3, 4, 5, 6, 9, 10, 17, 18):
            for v in (1, -1):
                add("one", s, gap, v)
        for gap in range(5):
            for v in (2, -2, 3, -3):
                add("two", s, gap, v)
        for gap in (8, 9, 62):
            add("run", s, gap, 5)
        for v in BOUNDARY_LEVELS:
            add("level", s, 0, v)
            add("level", s, 0, -v)
    for z in (62, 63):
        for v in (1, -7):
            b = np.zeros(64, np.int64)
            b[z] = v
            blocks.append(b)
            what.append(("end", z, 0, v))
    blocks.append(np.zeros(64, np.int64))
    what.append(("empty", 0, 0, 0))
    b = np.zeros(64, np.int64)
    b[0] = -3
    blocks.append(b)
    what.append(("dc", 0, 0, -3))
    return np.array(blocks), what


def dc_pred_scalar(m, l, ul, u, ur):
    """Spec 7.8 (Table 7.47 and the outlier rule) for one fragment, Python integers, division towards zero."""
    tdiv = lambda a, b: abs(a) // b * (1 if a >= 0 else -1)
    w = {0: (0, 0, 0, 0, 1), 1: (1, 0, 0, 0, 1), 2: (0, 1, 0, 0, 1), 3: (1, 0, 0, 0, 1), 4: (0, 0, 1, 0, 1), 5: (1, 0, 1, 0, 2),
         6: (0, 0, 1, 0, 1), 7: (29, -26, 29, 0, 32), 8: (0, 0, 0, 1, 1), 9: (75, 0, 0, 53, 128), 10: (0, 1, 0, 1, 2),
         11: (75, 0, 0, 53, 128), 12: (0, 0, 1, 0, 1), 13: (75, 0, 0, 53, 128), 14: (0, 3, 10, 3, 16), 15: (29, -26, 29, 0, 32)}[m]
    pred = tdiv(w[0] * l + w[1] * ul + w[2] * u + w[3] * ur, w[4])
    if m in (7, 15):
        if abs(pred - u) > 128:
            pred = u
        elif abs(pred - l) > 128:
            pred = l
        elif abs(pred - ul) > 128:
            pred = ul
    return pred


def dc_unpredict(geo, resid, ok=None, cl=None):
    """The quantised DCs [n] whose residuals are resid [n] (the decoder's direction, a scalar walk in raster order): where a fragment
    is not coded its DC stays what resid says."""
    n = geo.nfrags
    ok = np.ones(n, bool) if ok is None else ok
    cl = np.zeros(n, bool) if cl is None else cl
    dc = np.array(resid, np.int64)
    for g in geo.planes:
        nv, nh, o = g["nvfrags"], g["nhfrags"], g["froffset"]
        for fy in range(nv):
            for fx in range(nh):
                fi = o + fy * nh + fx
                if not ok[fi]:
                    continue
                m, v = 0, [0, 0, 0, 0]
                for k, (dy, dx) in enumerate(((0, -1), (-1, -1), (-1, 0), (-1, 1))):
                    y, x = fy + dy, fx + dx
                    if y >= 0 and 0 <= x < nh and ok[o + y * nh + x] and cl[o + y * nh + x] == cl[fi]:
                        m |= 1 << k
                        v[k] = int(dc[o + y * nh + x])
                dc[fi] += dc_pred_scalar(m, *v)
    return dc


def extreme_residuals():
    """Residual blocks [N, 64] at the ends of the range a pixel difference has: flat +-255, the three checkerboards of +-255, a single
    row or column of +-255 over zero and over the opposite sign."""
    y, x = np.mgrid[0:8, 0:8]
    out = [np.full((8, 8), 255), np.where((x + y) & 1, 255, -255), np.where(x & 1, 255, -255), np.where(y & 1, 255, -255)]
    for k in range(8):
        out += [np.where(y == k, 255, 0), np.where(x == k, 255, 0), np.where(y == k, 255, -255), np.where(x == k, 255, -255)]
    out = np.array(out).reshape(-1, 64)
    return np.concatenate([out, -out])


def coef_bound():
    """The largest magnitude the oracle's transform gives over extreme_residuals(): what the planted coefficients go up to."""
    return int(np.abs(oracle.fdct8x8_batch(extreme_residuals().astype(np.int16)).astype(np.int64)).max())


def dc_cases(geo, dc, ok, cl):
    """What the DC prediction of dc [n] with the flags ok and classes cl meets (a scalar walk): per plane the set of neighbour masks
    of the coded fragments; the fallbacks of the outlier rule ('u', 'l', 'ul', 'none'); the divisors that truncated a negative sum."""
    masks, fallbacks, negative = [set(), set(), set()], set(), set()
    for p, g in enumerate(geo.planes):
        nv, nh, o = g["nvfrags"], g["nhfrags"], g["froffset"]
        for fy in range(nv):
            for fx in range(nh):
                fi = o + fy * nh + fx
                if not ok[fi]:
                    continue
                m, v = 0, [0, 0, 0, 0]
                for k, (dy, dx) in enumerate(((0, -1), (-1, -1), (-1, 0), (-1, 1))):
                    y, x = fy + dy, fx + dx
                    if y >= 0 and 0 <= x < nh and ok[o + y * nh + x] and cl[o + y * nh + x] == cl[fi]:
                        m |= 1 << k
                        v[k] = int(dc[o + y * nh + x])
                masks[p].add(m)
                l, ul, u, ur = v
                num, den = {5: (l + u, 2), 10: (ul + ur, 2), 14: (3 * (ul + ur) + 10 * u, 16), 7: (29 * (l + u) - 26 * ul, 32),
                            15: (29 * (l + u) - 26 * ul, 32)}.get(m, (75 * l + 53 * ur, 128) if m in (9, 11, 13) else (0, 1))
                if num < 0 and num % den:
                    negative.add(den)
                if m in (7, 15):
                    q = abs(num) // 32 * (1 if num >= 0 else -1)
                    fallbacks.add("u" if abs(q - u) > 128 else "l" if abs(q - l) > 128 else "ul" if abs(q - ul) > 128 else "none")
    return masks, fallbacks, negative
