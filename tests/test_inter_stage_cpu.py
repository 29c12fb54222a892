"""tests/inter_stage_ref.py and the restatements it composes (enc_inter_ref, enc_modes_ref), held against things that are not
themselves: a scalar search written as plain loops, planted motion that must be found at no cost, the reference decoder's own DC
un-prediction, a rounding stated with fractions; and the refusals of thip_enc_inter_stage, which come before any device is touched.
No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import oracle
from tests import enc_inter_ref as IR
from tests import enc_modes_ref as MR
from tests import inter_stage_ref as R


# ---- a scalar search ------------------------------------------------------------------------------------------------------------
def axis(v):
    """(whole part towards zero, step of the second read) of a half-pel component"""
    whole = abs(v) // 2 * (1 if v >= 0 else -1)
    return whole, (0 if v % 2 == 0 else (1 if v > 0 else -1))


def scalar_search(src, ref, x0, y0, size):
    """One size x size block at (x0, y0): the candidates scanned in raster order, the least key (SAD, |mv|, index) kept; then its
    eight half-pel neighbours and itself (index 4 of the 3 x 3) the same way.  -> (full-pel index, SAD of vector 0, SAD, mvx, mvy)"""
    H, W = ref.shape
    ys, xs = np.arange(y0, y0 + size), np.arange(x0, x0 + size)
    blk = src[y0:y0 + size, x0:x0 + size].astype(np.int64)
    read = lambda dx, dy: ref[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)].astype(np.int64)
    best, s0 = None, None
    for ci in range(961):
        dx, dy = ci % 31 - 15, ci // 31 - 15
        sad = int(np.abs(blk - read(dx, dy)).sum())
        if dx == 0 and dy == 0:
            s0 = sad
        key = (sad, 2 * (abs(dx) + abs(dy)), ci)
        if best is None or key < best:
            best = key
    bdx, bdy = best[2] % 31 - 15, best[2] // 31 - 15
    hbest = None
    for k9 in range(9):
        mvx, mvy = 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1
        if k9 == 4:
            sad = best[0]
        else:
            (mx, mx2), (my, my2) = axis(mvx), axis(mvy)
            sad = int(np.abs(blk - ((read(mx, my) + read(mx + mx2, my + my2)) >> 1)).sum())   # the decoder's truncating average
        key = (sad, abs(mvx) + abs(mvy), k9)
        if hbest is None or key < hbest:
            hbest = key
    k9 = hbest[2]
    return best[2], s0, hbest[0], 2 * bdx + k9 % 3 - 1, 2 * bdy + k9 // 3 - 1


def content(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, shape).astype(np.int64), rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "near":   # the source a moved reference: low SADs, a clear winner
        ref = rng.integers(0, 256, shape, dtype=np.uint8)
        return np.roll(ref, (3, -5), (0, 1)).astype(np.int64), ref
    return R.tie_content(kind, shape, seed)


@pytest.mark.parametrize("kind", ["noise", "near", "flat", "two", ("x", 2, (2, 0)), ("y", 2, (0, 2))],
                         ids=lambda k: k if isinstance(k, str) else "%s%d" % k[:2])
@pytest.mark.parametrize("shape", [(16, 16), (16, 32), (48, 48)], ids=["16x16", "32x16", "48x48"])
def test_vectorised_searches_equal_a_scalar_one(shape, kind):
    """enc_inter_ref.search_stats, enc_modes_ref.search_all (macro blocks against PREV and GOLD, luma blocks) and tie_counts' winner
    against the plain loops, one block at a time.  (The period-2 content, moved by one whole pixel, ties candidates of equal |mv| on either side: the raster index decides.)"""
    src, prev = content(kind, shape, 7)
    gold = content(kind, shape, 8)[1]
    H, W = shape
    nmx = W // 16
    mvx, mvy, s0, si, smv = IR.search_stats(src, prev)
    ms = MR.search_all(src, prev, gold)
    bci = R.tie_counts(src, prev)[2]
    for mb in range((H // 16) * nmx):
        x0, y0 = (mb % nmx) * 16, (mb // nmx) * 16
        ci, a0, a, ax, ay = scalar_search(src, prev, x0, y0, 16)
        assert (ci, a0, a, ax, ay) == (bci[mb], s0[mb], smv[mb], mvx[mb], mvy[mb]), mb
        assert (a0, a, ax, ay) == (ms["s0"][mb], ms["smv"][mb], ms["mvx"][mb], ms["mvy"][mb]), mb
        _, g0, g, gx, gy = scalar_search(src, gold, x0, y0, 16)
        assert (g0, g, gx, gy) == (ms["g0"][mb], ms["gmv"][mb], ms["gvx"][mb], ms["gvy"][mb]), mb
        s4 = 0
        for b in range(4):
            _, _, sb, bx, by = scalar_search(src, prev, x0 + 8 * (b & 1), y0 + 8 * (b >> 1), 8)
            assert (bx, by) == (ms["bvx"][mb, b], ms["bvy"][mb, b]), (mb, b)
            s4 += sb
        assert s4 == ms["s4"][mb]
        blk = src[y0:y0 + 16, x0:x0 + 16]
        intra = sum(int(np.abs(q - ((int(q.sum()) + 32) >> 6)).sum()) for q in (blk[:8, :8], blk[:8, 8:], blk[8:, :8], blk[8:, 8:]))
        assert intra == si[mb] == ms["si"][mb]


@pytest.mark.parametrize("lam", [0, 1, 7, 100, 5000, 70000])
def test_decisions_follow_their_margins(lam):
    """The two restatements' decisions against the signs of the margins the equality tests are steered by."""
    src, prev = content("near", (48, 48), 3)
    src[:16] = content("noise", (16, 48), 5)[0]
    gold = np.roll(prev, 2, 1)
    st = R.search(src, prev)
    m1, m2 = R.margins5(st, lam)
    pix = IR.motion_search(src, prev, lam)[0]
    assert np.array_equal(pix, np.where(m2 < 0, R.INTRA, np.where(m1 < 0, R.MV, R.NOMV)))
    assert np.array_equal(R.decide5(st, lam)["pix"], pix)
    d = MR.motion_search(src, prev, gold, lam)
    m = d["margins"]
    inter = np.where(m[1] < 0, R.MV_FOUR, np.where(m[0] < 0, R.MV, R.NOMV))
    g = np.where(m[2] < 0, R.GOLDEN_MV, R.GOLDEN_NOMV)
    assert np.array_equal(d["pix"], np.where(m[4] < 0, R.INTRA, np.where(m[3] < 0, g, inter)))
    w = R.decide8(MR.search_all(src, prev, gold), lam)["words"]
    assert np.array_equal(w[:, 0] & 0xFF, d["pix"]) and w.dtype == np.uint32 and w.shape == (9, 4)


# ---- planted motion -------------------------------------------------------------------------------------------------------------
def test_every_planted_full_pel_vector_is_found_at_no_cost():
    src0, prev0, _ = R.every_candidate()
    mvx, mvy, s0, si, smv = IR.search_stats(src0, prev0)
    k = np.arange(961)
    assert (smv == 0).all() and np.array_equal(mvx, 2 * (k % 31 - 15)) and np.array_equal(mvy, 2 * (k // 31 - 15))
    assert (s0[k != 480] > 0).all() and s0[480] == 0


@pytest.mark.parametrize("full", [(0, 0), (15, 15), (-15, 15), (15, -15), (-15, -15), (0, -15), (15, 0), (7, -5)], ids=lambda v: "%d,%d" % v)
def test_every_planted_half_pel_vector_is_found_at_no_cost(full):
    """The nine half-pel vectors around 2 * full as the vector of the interior macro block of 48 x 48, by both restatements.  (A
    luma block's own search is not held to this: 64 noise pixels let the full-pel step of a diagonal vector at the range's edge, which
    has one full-pel neighbour in range, settle elsewhere -- the scalar search above agrees where it does.)"""
    rng = np.random.default_rng(5)
    prev0 = rng.integers(0, 256, (48, 48), dtype=np.uint8)
    for k9 in range(9):
        vx, vy = np.full((9, 4), 2 * full[0] + k9 % 3 - 1), np.full((9, 4), 2 * full[1] + k9 // 3 - 1)
        src0 = R.predicted(prev0, vx, vy)
        st = R.search(src0, prev0)
        assert (st["smv"][4], st["mvx"][4], st["mvy"][4]) == (0, vx[4, 0], vy[4, 0])
        best, _, _ = MR.full_pel(src0, prev0, False)
        got = MR.half_pel(src0, prev0, best, (np.arange(9) % 3) * 16, (np.arange(9) // 3) * 16, 16)
        assert (got[0][4], got[1][4], got[2][4]) == (0, vx[4, 0], vy[4, 0])


# ---- the chroma vectors of MV_FOUR ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_chroma_vectors_round_half_away_from_zero(fmt):
    geo = R.geometry(64, 64, fmt)
    rng = np.random.default_rng(2)
    n = 16
    bmv = rng.integers(-31, 32, (n, 4, 2))
    bmv[0], bmv[1] = [[-31, -1], [-31, 0], [-31, 0], [-29, 0]], [[1, 31], [0, 31], [0, 29], [1, 31]]
    fvx, fvy = MR.fragment_vectors(geo, np.full(n, R.MV_FOUR), np.zeros((n, 2), np.int64), bmv)

    def away(q):   # round(q), a tie away from zero
        f = abs(q)
        r = int(f) + (1 if f - int(f) >= Fraction(1, 2) else 0)
        return r if q >= 0 else -r
    ties = 0
    for p in (1, 2):
        g = geo.planes[p]
        for loc in range(g["nfrags"]):
            fy, fx = divmod(loc, g["nhfrags"])
            mb = int(geo.mb_of[g["froffset"] + loc])
            for c, fv in ((0, fvx), (1, fvy)):
                v = bmv[mb, :, c]
                if fmt == 0:
                    q = Fraction(int(v.sum()), 4)
                elif fmt == 2:
                    q = Fraction(int(v[2 * (fy & 1)] + v[2 * (fy & 1) + 1]), 2)
                else:
                    q = Fraction(int(v[2 * (fy & 1) + (fx & 1)]))
                ties += q < 0 and abs(q) % 1 == Fraction(1, 2)
                assert fv[g["froffset"] + loc] == away(q), (p, loc, c)
    assert fmt == 3 or ties > 0
    g0 = geo.planes[0]
    for loc in range(g0["nfrags"]):
        fy, fx = divmod(loc, g0["nhfrags"])
        assert (fvx[loc], fvy[loc]) == tuple(bmv[geo.mb_of[loc], 2 * (fy & 1) + (fx & 1)])


# ---- the DC residuals, inverted by the decoder ------------------------------------------------------------------------------------
REFI = np.array([3, oracle.FRAME_SELF, oracle.FRAME_PREV, oracle.FRAME_GOLD], np.uint8)   # by class; 3: an uncoded fragment's


@pytest.mark.parametrize("classes", [2, 3])
@pytest.mark.parametrize("geo_name,kind", [(g, k) for g in R.GEOS for k in R.MAPS if k != "far" or g == "1536x1024"])
def test_decoder_inverts_dc_residuals(geo_name, kind, classes):
    """The residuals in oracle.State.dc, the classes in coded and refi: dc_unpredict() gives the quantised DCs back."""
    fw, fh, fmt = R.GEOS[geo_name]
    geo, cm, dcq = R.dc_case(geo_name, kind, classes)
    dcr = R.dc(geo, cm, dcq, classes)
    assert (dcr[cm == 0] == 0).all()
    st = oracle.State(fw, fh, fmt)
    try:
        st.coded[:] = cm != 0
        st.refi[:] = REFI[cm]
        st.dc[:] = dcr
        st.dc_unpredict()
        assert np.array_equal(st.dc[cm != 0], dcq[cm != 0])
    finally:
        st.close()


def test_stage_c_composes_the_encoders_own_frame():
    """code() over the modes of a restated inter frame gives the blocks that frame's packet was written from: the same coded set,
    and DC residuals the decoder inverts."""
    geo = R.geometry(64, 48, 0)
    rng = np.random.default_rng(4)
    prev = [rng.integers(0, 256, (g["height"], g["width"]), dtype=np.uint8) for g in geo.planes]
    src = [np.clip(np.roll(a, (1, 2), (0, 1)).astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255) for a in prev]
    tab = R.tables_flat(24)
    d = R.decide5(R.search(src[0], prev[0]), 24)
    c = R.code(geo, src, prev, None, d["pix"], d["mv"], None, tab, 2)
    assert c["levels"].shape == (geo.nfrags, 64) and np.array_equal(c["levels"][:, 0], c["dcq"][geo.coded_order])
    assert set(np.unique(c["cmap"])) <= {0, 1, 2} and (c["dcr"][c["cmap"] == 0] == 0).all()
    st = oracle.State(64, 48, 0)
    try:
        st.coded[:] = c["cmap"] != 0
        st.refi[:] = REFI[c["cmap"]]
        st.dc[:] = c["dcr"]
        st.dc_unpredict()
        assert np.array_equal(st.dc[c["cmap"] != 0], c["dcq"][c["cmap"] != 0])
    finally:
        st.close()


# ---- the entry's refusals ---------------------------------------------------------------------------------------------------------
A = 0x10000   # a device address nobody reads: every case below is refused before a device is touched
OK_KW = dict(frame=(64, 48), pixel_fmt=0, stages=7, classes=2, pic=(1, 2, 61, 45), lam=5, src=[A + 1] * 3, src_pitch=[63, 33, 33],
             prev=[A] * 3, ref_pitch=[64, 32, 32], dequant=np.ones(384), stats=A, words=A, levels=A, dcq=A, cmap=A, dcr=A)
REFUSALS = [
    ("no stage", dict(stages=0), -10), ("unknown stage", dict(stages=16), -10), ("DC with another", dict(stages=9), -10),
    ("negative stages", dict(stages=-1), -10),
    ("width 0", dict(frame=(0, 48)), -10), ("height not a multiple of 16", dict(frame=(64, 40)), -10),
    ("width 2^20", dict(frame=(1 << 20, 48)), -10), ("too many fragments", dict(frame=(65536, 65536), pixel_fmt=3), -10),
    ("format 1", dict(pixel_fmt=1), -10), ("format 4", dict(pixel_fmt=4), -10),
    ("classes 1", dict(classes=1), -10), ("classes 4", dict(classes=4), -10),
    ("gold with classes 2", dict(gold=[A] * 3), -10), ("classes 3 without gold", dict(classes=3), -1),
    ("classes 3, one gold plane missing", dict(classes=3, gold=[A, None, A]), -1),
    ("picture beyond the frame", dict(pic=(4, 2, 61, 45)), -10), ("picture height 0", dict(pic=(1, 2, 61, 0)), -10),
    ("negative pic_x", dict(pic=(-1, 2, 61, 45)), -10),
    ("no source plane", dict(src=[A, None, A]), -1), ("no PREV plane", dict(prev=[None, A, A]), -1),
    ("source pitch below the picture", dict(src_pitch=[60, 33, 33]), -10), ("chroma source pitch below", dict(src_pitch=[63, 30, 33]), -10),
    ("reference pitch below the frame", dict(ref_pitch=[63, 32, 32]), -10), ("reference pitch 2^31", dict(ref_pitch=[1 << 31, 32, 32]), -10),
    ("negative lambda", dict(lam=-1), -10), ("lambda too large", dict(lam=(1 << 24) + 1), -10),
    ("no stats", dict(stats=None), -1), ("no words", dict(words=None), -1), ("no dequant", dict(dequant=None), -1),
    ("a step of 0", dict(dequant=np.r_[np.ones(383), 0]), -10), ("a step of 32768", dict(dequant=np.r_[32768, np.ones(383)]), -10),
    ("from-stats words without SEARCH", dict(stages=6, words_from_stats=A), -10),
    ("from-stats words without DECIDE", dict(stages=5, words_from_stats=A), -10),
    ("from-stats words with classes 3", dict(classes=3, gold=[A] * 3, words_from_stats=A), -10),
    ("stats misaligned", dict(stats=A + 8), -10), ("words misaligned", dict(words=A + 2), -10),
    ("16-byte words misaligned", dict(classes=3, gold=[A] * 3, words=A + 4), -10),
    ("from-stats words misaligned", dict(words_from_stats=A + 1), -10),
    ("levels misaligned", dict(levels=A + 8), -10), ("dcq misaligned", dict(dcq=A + 1), -10), ("dcr misaligned", dict(dcr=A + 1), -10),
    ("DC without cmap", dict(stages=8, cmap=None), -1), ("DC without dcq", dict(stages=8, dcq=None), -1),
    ("DC without dcr", dict(stages=8, dcr=None), -1),
]


@pytest.mark.parametrize("what,change,rc", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refusals(what, change, rc):
    from theora_amd.encoder import inter_stage
    assert inter_stage(**dict(OK_KW, **change)) == rc, what


def test_entry_takes_a_wrong_dequant_size_for_the_callers_mistake():
    from theora_amd.encoder import inter_stage
    with pytest.raises(ValueError):
        inter_stage(**dict(OK_KW, dequant=np.ones(192)))
