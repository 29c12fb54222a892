"""inter_stage_ref.py -- TEST INFRASTRUCTURE: the device stage of a th_encode_* inter frame, one function per stage, as
thip_enc_inter_stage (include/theora_hip.h) hands its results out.  Nothing is restated here: the searches, the decisions, the
prediction and the DC residuals are enc_inter_ref's and enc_modes_ref's, the transform and the quantiser the oracle's; this module
composes them over given arrays and packs the results as the kernels' words.

Everything is in bitstream coordinates: planes [H, W] with row 0 the BOTTOM row, macro blocks and fragments in raster order from
the bottom, vectors in half pixels with y pointing up.  src: the three frame-sized planes the encoder transforms (the picture
clamped outward, enc_ref.frame_planes flipped); prev, gold: the references' three planes.
"""
import functools

import numpy as np

import oracle
from tests import enc_inter_ref as IR
from tests import enc_modes_ref as MR
from tests.enc_inter_ref import predict

NOMV, INTRA, MV, GOLDEN_NOMV, GOLDEN_MV, MV_FOUR = MR.NOMV, MR.INTRA, MR.MV, MR.GOLDEN_NOMV, MR.GOLDEN_MV, MR.MV_FOUR


def frame_src(planes, fw, fh, fmt, pic):
    """The source as the stage functions take it, from picture- or frame-sized planes (rows top first)."""
    from tests import enc_ref
    return [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, fw, fh, fmt, pic)]


# ---- the words ----------------------------------------------------------------------------------------------------------------
def _b(v):
    return np.asarray(v, np.int64) & 0xFF


def pack_stats(s0, smv, si, mvx, mvy):
    """k_rate_me's words [nmbs, 4]."""
    return np.stack([s0, smv, si, _b(mvx) | _b(mvy) << 8], 1).astype(np.uint32)


def pack_words5(pix, mvx, mvy):
    """k_enc_me's words [nmbs]: mode | mvx << 8 | mvy << 16."""
    return (np.asarray(pix, np.int64) | _b(mvx) << 8 | _b(mvy) << 16).astype(np.uint32)


def pack_words8(pix, mv, bmv, gv):
    """k_enc_me_all's words [nmbs, 4]: mode | vector << 8; block vectors 0, 1; 2, 3; the GOLD search's vector."""
    pk = lambda v: _b(v[..., 0]) | _b(v[..., 1]) << 8
    mv, bmv, gv = np.asarray(mv, np.int64), np.asarray(bmv, np.int64), np.asarray(gv, np.int64)
    return np.stack([np.asarray(pix, np.int64) | pk(mv) << 8, pk(bmv[:, 0]) | pk(bmv[:, 1]) << 16, pk(bmv[:, 2]) | pk(bmv[:, 3]) << 16,
                     pk(gv)], 1).astype(np.uint32)


# ---- (a), (b): the search and the decision ---------------------------------------------------------------------------------------
def search(src0, prev0):
    """Stage (a): dict(s0, smv, si, mvx, mvy) of the five-mode search against PREV (enc_inter_ref.search_stats), and k_rate_me's
    words as `words`."""
    mvx, mvy, s0, si, smv = IR.search_stats(src0, prev0)
    return dict(s0=s0, smv=smv, si=si, mvx=mvx, mvy=mvy, words=pack_stats(s0, smv, si, mvx, mvy))


def search_of(ms):
    """search()'s dict from enc_modes_ref.search_all's: its PREV macro-block search is the five-mode search (the tests of
    tests/test_inter_stage_cpu.py hold the two restatements against each other)."""
    d = {k: ms[k] for k in ("s0", "smv", "si", "mvx", "mvy")}
    return dict(d, words=pack_stats(d["s0"], d["smv"], d["si"], d["mvx"], d["mvy"]))


def decide5(st, lam):
    """Stage (b), five modes: k_enc_me's words from search()'s dict (enc_inter_ref.decide's mode and vector)."""
    pix, mvx, mvy = IR.decide((st["mvx"], st["mvy"], st["s0"], st["si"], st["smv"]), lam)[:3]
    return dict(pix=pix, mv=np.stack([mvx, mvy], 1), words=pack_words5(pix, mvx, mvy))


def decide8(ms, lam):
    """Stage (b), eight modes: k_enc_me_all's words from enc_modes_ref.search_all's dict."""
    d = MR.decide(ms, lam)
    d["words"] = pack_words8(d["pix"], d["mv"], d["bmv"], np.stack([ms["gvx"], ms["gvy"]], 1))
    return d


# ---- (c): prediction, transform, quantiser, then the DC --------------------------------------------------------------------------
def coefficients_of(geo, src, prev, gold, fpix, fvx, fvy):
    """Every fragment's fDCT (raster order, zig-zag, int16) and its table type: the residual against the prediction of its pixel mode
    fpix [nfrags] with its vector (fvx, fvy) from PREV or GOLD (gold may be None without GOLD modes), 128 for INTRA (prev may be None
    when every block is INTRA)."""
    fgold = (fpix == GOLDEN_NOMV) | (fpix == GOLDEN_MV)
    dct = np.zeros((geo.nfrags, 64), np.int16)
    qti_of = np.zeros(geo.nfrags, np.int64)
    for p, g in enumerate(geo.planes):
        nh = g["nhfrags"]
        fi = g["froffset"] + np.arange(g["nfrags"])
        fy, fx = (fi - g["froffset"]) // nh, (fi - g["froffset"]) % nh
        r = np.arange(8)
        Y = fy[:, None, None] * 8 + r[None, :, None]
        X = fx[:, None, None] * 8 + r[None, None, :]
        qx, qy = p > 0 and geo.hdec, p > 0 and geo.vdec
        vx, vy = fvx[fi][:, None, None], fvy[fi][:, None, None]
        intra = fpix[fi] == INTRA
        if prev is None:
            assert intra.all()
            pred = np.full(Y.shape[:1] + (8, 8), 128, np.int64)
        else:
            pred = predict(prev[p], X, Y, vx, vy, qx, qy)
            if gold is not None:
                pred = np.where(fgold[fi][:, None, None], predict(gold[p], X, Y, vx, vy, qx, qy), pred)
            pred[intra] = 128
        res = (src[p][Y, X] - pred).reshape(-1, 64)
        qti_of[fi] = np.where(intra, 0, 1)
        dct[fi] = oracle.fdct8x8_batch(res.astype(np.int16))
    return dct, qti_of


def levels_of(geo, src, prev, gold, fpix, fvx, fvy, tabs):
    """Every fragment's quantised levels (raster order, zig-zag) and its table type: the prediction of its pixel mode fpix [nfrags]
    with its vector (fvx, fvy) from PREV or GOLD (gold may be None without GOLD modes), 128 for INTRA; tabs[(qti, plane)]: the
    zig-zag tables.  (The block loop of InterEncoder._inter and ModesEncoder._inter, which call this.)"""
    dct, qti_of = coefficients_of(geo, src, prev, gold, fpix, fvx, fvy)
    lev = np.zeros((geo.nfrags, 64), np.int64)
    for p, g in enumerate(geo.planes):
        fi = g["froffset"] + np.arange(g["nfrags"])
        for t in range(2):
            sel = qti_of[fi] == t
            if sel.any():
                q, _ = oracle.quantize_batch(dct[fi[sel]], tabs[(t, p)].astype(np.uint16))
                lev[fi[sel]] = q
    return lev, qti_of


def code(geo, src, prev, gold, pix, mv, bmv, dequant, nclasses):
    """Stage (c) over the macro blocks' modes pix [nmbs], vectors mv [nmbs, 2] and block vectors bmv [nmbs, 4, 2] (None: no
    MV_FOUR); dequant [2][3][64] zig-zag.  dict(levels [nfrags, 64] in CODED order, dcq, cmap, dcr [nfrags] raster, fvx, fvy)."""
    pix, mv = np.asarray(pix, np.int64), np.asarray(mv, np.int64)
    bmv = np.zeros((len(pix), 4, 2), np.int64) if bmv is None else np.asarray(bmv, np.int64)
    fvx, fvy = MR.fragment_vectors(geo, pix, mv, bmv)
    fpix = pix[geo.mb_of]
    dq = np.asarray(dequant, np.int64).reshape(2, 3, 64)
    tabs = {(t, p): dq[t, p] for t in range(2) for p in range(3)}
    lev, qti_of = levels_of(geo, src, prev, gold, fpix, fvx, fvy, tabs)
    fgold = (fpix == GOLDEN_NOMV) | (fpix == GOLDEN_MV)
    cls = np.where(qti_of == 0, 1, np.where(fgold, 3, 2))
    assert nclasses == 3 or not fgold.any()
    coded = (fpix != NOMV) | (lev != 0).any(1)
    dcr = MR.dc_residuals(geo, lev, coded, cls, nclasses)
    return dict(levels=lev[geo.coded_order].astype(np.int16), dcq=lev[:, 0].astype(np.int16), cmap=(coded * cls).astype(np.uint8),
                dcr=dcr.astype(np.int16), fvx=fvx, fvy=fvy, lev=lev)


# ---- (d): the DC alone ------------------------------------------------------------------------------------------------------------
def dc(geo, cmap, dcq, nclasses):
    """Stage (d): dcr [nfrags] (int16; 0 where cmap is 0) of the class map cmap (0 uncoded, else the class) and the quantised DCs."""
    cmap = np.asarray(cmap, np.int64)
    return MR.dc_residuals(geo, np.asarray(dcq, np.int64)[:, None], cmap != 0, cmap, nclasses).astype(np.int16)


# ---- what the tests ask of the reference besides its results ----------------------------------------------------------------------
def margins5(st, lam):
    """Left side less right side of the two inequalities of the five-mode rule over search()'s dict."""
    m1 = st["smv"] + lam - st["s0"]
    return [m1, st["si"] + 4 * lam - np.where(m1 < 0, st["smv"], st["s0"])]


def tie_counts(src0, ref0):
    """How many full-pel candidates stand at the least SAD of each macro block; how many of the nine half-pel candidates around the
    full-pel winner stand at the least SAD of the nine; and the winner's raster index among the 961."""
    s = src0.astype(np.int64)
    H, W = s.shape
    nmy, nmx = H // 16, W // 16
    n = nmy * nmx
    best = MR.full_pel(s, ref0, False)[0]
    pad = np.pad(ref0, 16, mode="edge").astype(np.int64)
    sad = np.stack([np.abs(s - pad[16 + dy:16 + dy + H, 16 + dx:16 + dx + W]).reshape(nmy, 16, nmx, 16).sum((1, 3)).reshape(-1)
                    for dy in range(-15, 16) for dx in range(-15, 16)])
    assert np.array_equal(sad.min(0), best >> 32)
    bci = best & 0xFFFF
    bdx, bdy = bci % 31 - 15, bci // 31 - 15
    r = np.arange(16)
    Y = ((np.arange(n) // nmx) * 16)[:, None, None] + r[None, :, None]
    X = ((np.arange(n) % nmx) * 16)[:, None, None] + r[None, None, :]
    hp = np.stack([np.abs(s[Y, X] - predict(ref0, X, Y, (2 * bdx + k9 % 3 - 1)[:, None, None], (2 * bdy + k9 // 3 - 1)[:, None, None],
                                            False, False)).sum((1, 2)) for k9 in range(9)])
    return (sad == sad.min(0)).sum(0), (hp == hp.min(0)).sum(0), bci


def tables_qi(setup, qi):
    """[2][3][64]: the zig-zag intra then inter tables of a setup header (enc_ref.SetupParams) at qi."""
    from tests.enc_ref import ZIGZAG
    return np.array([[setup.qmat(t, p, qi)[ZIGZAG] for p in range(3)] for t in range(2)], np.uint16)


def tables_flat(step=1):
    """The flat table of one step; 1 is the finest the quantiser is defined for (thip_fdct.h: quant_recip takes a step that is not
    zero), and with it a level is the coefficient itself: a one-pixel rounding difference moves a level."""
    return np.full((2, 3, 64), step, np.uint16)


# ---- content ------------------------------------------------------------------------------------------------------------------
def displaced(ref0, dx, dy):
    """Luma source (bitstream rows) whose macro block k is ref0 displaced by (dx[k], dy[k]) whole pixels, coordinates clamped."""
    H, W = ref0.shape
    nmx = W // 16
    y, x = np.mgrid[0:H, 0:W]
    mb = (y // 16) * nmx + x // 16
    return ref0[np.clip(y + np.asarray(dy)[mb], 0, H - 1), np.clip(x + np.asarray(dx)[mb], 0, W - 1)].astype(np.int64)


def predicted(ref0, bvx, bvy):
    """Luma source whose 8 x 8 block b of macro block k is the decoder's prediction from ref0 with the half-pel vector
    (bvx[k, b], bvy[k, b]) (blocks 2 i + j, i the row from the bottom)."""
    H, W = ref0.shape
    nmx = W // 16
    y, x = np.mgrid[0:H, 0:W]
    mb = (y // 16) * nmx + x // 16
    b = 2 * ((y >> 3) & 1) + ((x >> 3) & 1)
    return predict(ref0, x, y, np.asarray(bvx)[mb, b], np.asarray(bvy)[mb, b], False, False)


def every_candidate(seed=0):
    """The 496 x 496 case: a noise PREV, the source of macro block (i, j) PREV displaced by (j - 15, i - 15); GOLD holds the source's
    macro blocks pasted at the transposed displacement (i - 15, j - 15), the part in the frame, over noise.  (src0, prev0, gold0)."""
    rng = np.random.default_rng(seed)
    prev0 = rng.integers(0, 256, (496, 496), dtype=np.uint8)
    k = np.arange(961)
    src0 = displaced(prev0, k % 31 - 15, k // 31 - 15)
    gold0 = rng.integers(0, 256, (496, 496), dtype=np.uint8)
    for i in range(31):
        for j in range(31):
            y0, x0 = 16 * i + (j - 15), 16 * j + (i - 15)
            ys, xs = slice(max(y0, 0), min(y0 + 16, 496)), slice(max(x0, 0), min(x0 + 16, 496))
            gold0[ys, xs] = src0[ys.start - (j - 15):ys.stop - (j - 15), xs.start - (i - 15):xs.stop - (i - 15)]
    return src0, prev0, gold0


def tie_content(kind, shape, seed=0):
    """(src0, prev0) full of equal SADs.  kind: "flat"; ("x" | "y" | "xy", period, (sx, sy)): PREV periodic along that axis (both:
    a tiled period x period cell), random along the other, the source the prediction of the half-pel vector (sx, sy) from the same
    pattern continued beyond the frame (an odd component along the period makes both half-pel neighbours equal); "two": two-valued
    random pixels."""
    rng = np.random.default_rng(seed)
    H, W = shape
    if kind == "flat":
        return np.full(shape, 77, np.int64), np.full(shape, 77, np.uint8)
    if kind == "two":
        return rng.choice([40, 200], shape).astype(np.int64), rng.choice([40, 200], shape).astype(np.uint8)
    axis, per, (sx, sy) = kind
    y, x = np.mgrid[0:H + 32, 0:W + 32]
    if axis == "x":
        big = rng.integers(0, 256, (H + 32, per), dtype=np.uint8)[y, x % per]
    elif axis == "y":
        big = rng.integers(0, 256, (per, W + 32), dtype=np.uint8)[y % per, x]
    else:
        big = rng.integers(0, 256, (per, per), dtype=np.uint8)[y % per, x % per]
    yy, xx = np.mgrid[16:16 + H, 16:16 + W]
    return predict(big, xx, yy, sx, sy, False, False), np.ascontiguousarray(big[16:16 + H, 16:16 + W])


# ---- the DC stage's geometries and class maps ------------------------------------------------------------------------------------
@functools.lru_cache(None)
def geometry(fw, fh, fmt):
    return IR.Geometry(fw, fh, fmt)


GEOS = {"16x16": (16, 16, 0), "48x32": (48, 32, 2), "272x16": (272, 16, 0), "1536x1024": (1536, 1024, 3)}
MAPS = ["dense", "half", "sparse", "single", "far", "edges"]


def class_map(kind, geo, classes, rng):
    """cmap [nfrags] of a kind (module docstring, D): 0 uncoded, else the class."""
    n = geo.nfrags
    cm = np.zeros(n, np.uint8)
    cls = rng.integers(1, classes + 1, n)
    if kind == "dense":
        cm[:] = cls
    elif kind == "half":
        cm[:] = np.where(rng.random(n) < 0.5, cls, 0)
    elif kind == "sparse":
        cm[:] = np.where(rng.random(n) < 1 / 300, cls, 0)
        cm[rng.integers(0, n)] = 1
    elif kind == "single":
        cm[n // 2] = classes
    elif kind == "far":
        # class 1 only in chunk 0 and next past the 257th chunk (another plane: the fall-back is cut); class 2 first in chunk 258
        # and next in chunk 285 of the same plane (the fall-back is found by the second pass over the earlier chunks); the last
        # class, if a third, fills the chunks between sparsely
        assert n > 286 * 256
        cm[[5, 200]] = 1
        cm[[270 * 256 + 17, 270 * 256 + 40]] = 1
        cm[[258 * 256 + 3, 285 * 256 + 77, 285 * 256 + 79]] = 2
        if classes == 3:
            cm[np.arange(300, 257 * 256, 997)] = 3
    else:
        # a class's last coded fragment before an isolated one: the last of a chunk, the first of a chunk, the last of the
        # previous plane, the first of the plane
        for p in (1, 2):
            o, np_ = geo.froff[p], geo.planes[p]["nfrags"]
            cm[o - 1] = 1                      # the previous plane's last
            if np_ > 2:
                cm[o + 2] = 1                  # isolated: falls back to nothing of this plane
            cm[o] = 2                          # the plane's first
            if np_ > 3 and classes == 3:
                cm[o + 3] = 3
        for c in range(256, n - 8, 256):
            if c in geo.froff:
                continue
            if c // 256 % 3 == 0:
                cm[[c - 1, c + 5]] = 2         # the last of a chunk, then an isolated one in the next
            elif c // 256 % 3 == 1:
                cm[[c, c + 6]] = 1             # the first of a chunk, then an isolated one in it
    return cm


def dc_case(geo_name, kind, classes):
    fw, fh, fmt = GEOS[geo_name]
    geo = geometry(fw, fh, fmt)
    rng = np.random.default_rng(len(kind) * 100 + classes * 10 + fw)
    cm = class_map(kind, geo, classes, rng)
    # half of the DCs anywhere in +-2000, half within +-120: neighbours far apart and close together both occur, which the three
    # 128-range corrections need
    dcq = np.where(rng.random(geo.nfrags) < 0.5, rng.integers(-2000, 2001, geo.nfrags), rng.integers(-120, 121, geo.nfrags)).astype(np.int16)
    nz = np.flatnonzero(cm)
    a = int(nz[0])
    b = int(nz[-1]) if len(nz) > 1 else (a + 1) % geo.nfrags
    dcq[a], dcq[b] = -2000, 2000
    return geo, cm, dcq
