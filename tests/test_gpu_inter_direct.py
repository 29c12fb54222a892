"""The inter stage of th_encode_* driven directly, through thip_enc_inter_stage: the motion search (enc_me_search in k_rate_me and
k_enc_me, k_enc_me_all, k_enc_mb_modes), the prediction and the quantiser (enc_block_pred, enc_pred_block, enc_residual_row in
k_enc_inter_fq and k_enc_inter_fq_all) and the DC residuals (k_enc_inter_dc, k_enc_inter_dc3), on inputs no picture sequence
produces: every one of the 961 candidates planted, every half-pel neighbour at the edge of the range, content full of ties, lambda at,
one below and one above the equality of every inequality of the two mode rules, vectors that leave the frame on every side of every
plane, chroma averages at negative ties, class maps that put the "last coded DC of its class" across chunk and plane edges.

Every comparison is exact equality with tests/inter_stage_ref.py (the restatements of enc_inter_ref / enc_modes_ref and the oracle's
transform, composed).  Every "this case reaches that edge" is asserted from the reference inside the test.  The source always has an
odd pitch and an odd base address, the references a pitch that is no multiple of four; every output lies in front of a guard that
must come back untouched."""
import functools

import numpy as np
import pytest

from tests import enc_inter_ref as IR
from tests import enc_modes_ref as MR
from tests import inter_stage_ref as R

pytestmark = pytest.mark.gpu

SEARCH, DECIDE, CODE, DC = 1, 2, 4, 8
_GUARD = 64


geometry = R.geometry


@functools.lru_cache(None)
def tables(kind):
    if kind == "flat1":
        return R.tables_flat(1)
    from tests import enc_ref
    from theora_amd.encoder import Encoder
    e = Encoder(16, 16, 0, 63)
    t = R.tables_qi(enc_ref.SetupParams(e.header_packets()[2]), 63)
    e.close()
    return t


def _upload(planes, pad, base):
    """Planes (numpy uint8, rows in the order the entry reads them) on the device with pitch width + pad behind `base` spare bytes.
    -> (tensors to keep, addresses, pitches)"""
    import torch
    keep, ptrs, pitches = [], [], []
    for a in planes:
        h, w = a.shape
        pitch = w + pad
        buf = np.full(base + h * pitch, 0xA5, np.uint8)
        buf[base:].reshape(h, pitch)[:, :w] = a
        t = torch.from_numpy(buf).cuda()
        keep.append(t)
        ptrs.append(t.data_ptr() + base)
        pitches.append(pitch)
    return keep, ptrs, pitches


def run(frame, fmt, stages, classes, src=None, pic=None, prev=None, gold=None, lam=0, dequant=None, words=None, cmap=None, dcq=None,
        from_stats=False, want=("levels", "dcq", "cmap", "dcr"), expect_rc=0):
    """One call of the entry.  src: picture-sized planes, rows top first; prev, gold: frame-sized planes in bitstream row order.
    -> dict of numpy arrays (stats [nmbs, 4], words [nmbs] or [nmbs, 4], from_stats [nmbs], levels [n, 64], dcq, cmap, dcr [n])."""
    import torch
    from theora_amd.encoder import inter_stage
    geo = geometry(frame[0], frame[1], fmt)
    n, nmbs = geo.nfrags, (frame[0] // 16) * (frame[1] // 16)
    keep, kw = [], {}
    if src is not None:
        k, kw["src"], kw["src_pitch"] = _upload([np.ascontiguousarray(a, np.uint8) for a in src], 1 if src[0].shape[1] % 2 == 0 else 2, 1)
        keep += k
    if prev is not None:
        k, kw["prev"], kw["ref_pitch"] = _upload(prev, 5, 0)
        keep += k
    if gold is not None:
        k, kw["gold"], pitch = _upload(gold, 5, 0)
        keep += k
        assert pitch == kw["ref_pitch"]
    sizes = dict(stats=nmbs * 16, words=nmbs * (16 if classes == 3 else 4), words_from_stats=nmbs * 4, levels=n * 128, dcq=n * 2, cmap=n,
                 dcr=n * 2)
    outs = {}

    def out(name, init=None):
        t = torch.full((sizes[name] + _GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        if init is not None:
            t[:sizes[name]] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)).cuda()
        outs[name] = t
        kw[name] = t.data_ptr()
    if stages & SEARCH:
        out("stats")
    if stages & (DECIDE | CODE):
        out("words", None if stages & DECIDE else words)
    if from_stats:
        out("words_from_stats")
    if stages & CODE:
        for name in want:
            out(name)
    if stages & DC:
        out("cmap", np.asarray(cmap, np.uint8))
        out("dcq", np.asarray(dcq, np.int16))
        out("dcr")
    torch.cuda.synchronize()
    rc = inter_stage(frame, fmt, stages, classes, pic=pic, lam=lam, dequant=dequant, **kw)
    assert rc == expect_rc, rc
    del keep
    res = {}
    dt = dict(stats=np.uint32, words=np.uint32, words_from_stats=np.uint32, levels=np.int16, dcq=np.int16, cmap=np.uint8, dcr=np.int16)
    for name, t in outs.items():
        a = t.cpu().numpy()
        assert (a[sizes[name]:] == 0x5A).all(), "%s: written beyond its end" % name
        a = a[:sizes[name]].view(dt[name])
        res[name] = a.reshape(-1, 4) if name == "stats" or (name == "words" and classes == 3) else a.reshape(-1, 64) if name == "levels" else a
    if "words_from_stats" in res:
        res["from_stats"] = res.pop("words_from_stats")
    return res


def top(planes):
    """Bitstream-order planes as the source the entry takes (rows top first)."""
    return [np.flipud(np.asarray(a)).astype(np.uint8) for a in planes]


def same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError("%s: %d of %d differ, first at %s: %r for %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                             ref[tuple(bad[0])]))


def chroma_of(shape, fmt, rng):
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    return [rng.integers(0, 256, (shape[0] >> vd, shape[1] >> hd), dtype=np.uint8) for _ in range(2)]


def check_search(src0, prev0, gold0, lams, fmt=0, st=None, ms=None):
    """Luma src0 (bitstream rows) through k_rate_me, k_enc_me, k_enc_mb_modes and k_enc_me_all at every lambda of lams, against the
    reference.  -> (search's dict, search_all's dict)"""
    H, W = src0.shape
    rng = np.random.default_rng(W * 7 + H)
    ch = chroma_of((H, W), fmt, rng)
    src = top([src0] + ch)
    prev, gold = [prev0] + ch, [gold0] + ch
    st = st or R.search(src0, prev0)
    ms = ms or MR.search_all(src0, prev0, gold0)
    for k in ("s0", "smv", "si", "mvx", "mvy"):
        assert np.array_equal(st[k], ms[k]), k   # (one search, stated twice in the reference)
    for lam in lams:
        got = run((W, H), fmt, SEARCH | DECIDE, 2, src=src, prev=prev, lam=lam, from_stats=True)
        same(got["stats"], st["words"], "k_rate_me")
        ref5 = R.decide5(st, lam)["words"]
        same(got["words"], ref5, "k_enc_me, lambda %d" % lam)
        same(got["from_stats"], ref5, "k_enc_mb_modes, lambda %d" % lam)
        got = run((W, H), fmt, DECIDE, 3, src=src, prev=prev, gold=gold, lam=lam)
        same(got["words"], R.decide8(ms, lam)["words"], "k_enc_me_all, lambda %d" % lam)
    return st, ms


# ---- S. the search ----------------------------------------------------------------------------------------------------------------
def test_every_candidate(hip):
    """961 work groups, one per full-pel candidate, those that point out of the frame included: the last LDS word of a window row,
    every alignbyte shift, +-30 as bytes.  In GOLD the displacements are transposed."""
    src0, prev0, gold0 = R.every_candidate()
    ms = MR.search_all(src0, prev0, gold0)
    st = R.search_of(ms)   # (at this size the five-mode restatement's own search is a second too many; every other case runs it)
    k = np.arange(961)
    assert (st["smv"] == 0).all()
    assert np.array_equal(st["mvx"], 2 * (k % 31 - 15)) and np.array_equal(st["mvy"], 2 * (k // 31 - 15))
    check_search(src0, prev0, gold0, [0, 40], st=st, ms=ms)
    gv = set(zip(ms["gvx"].tolist(), ms["gvy"].tolist()))
    assert len(gv) >= 900 and {abs(x) for x, _ in gv} >= set(range(0, 31, 2)) and np.mean(ms["gvx"] == ms["mvy"]) > 0.9
    assert (R.decide8(ms, 0)["pix"] == R.MV).sum() > 900   # (the vector is in the word)


FULL = [(0, 0), (15, 15), (15, -15), (-15, 15), (-15, -15), (0, 15), (0, -15), (15, 0), (-15, 0), (7, -5)]


@pytest.mark.parametrize("shape", [(16, 16), (48, 16), (16, 48), (48, 48)], ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("full", FULL, ids=lambda v: "%d,%d" % v)
def test_half_pel(hip, full, shape):
    """The source is the decoder's prediction for each of the nine half-pel vectors around 2 * full (+-31 at the corners of the
    range), one per macro block, rotated through the macro blocks from launch to launch; then with each luma block given its own of the
    nine.  16 x 16: the whole window outside the block is clamped; 48 x 48: corner, edge and interior blocks."""
    # (+-31 is a negative byte in the words on one side, the last half-pel read of the window on the other)
    H, W = shape
    n = (H // 16) * (W // 16)
    rng = np.random.default_rng(5)
    prev0 = rng.integers(0, 256, shape, dtype=np.uint8)
    gold0 = rng.integers(0, 256, shape, dtype=np.uint8)
    seen = set()
    for rot in ((0, 2, 4, 6, 8) if n == 9 else range(0, 9, min(n, 3))):
        k9 = (np.arange(n)[:, None] + rot + np.array([0, 2, 5, 6])[None, :]) % 9   # [n, 4]: the four blocks' offsets
        for four in (False, True):
            kk = k9 if four else np.repeat(k9[:, :1], 4, 1)
            vx, vy = 2 * full[0] + kk % 3 - 1, 2 * full[1] + kk // 3 - 1
            src0 = R.predicted(prev0, vx, vy)
            st, ms = check_search(src0, prev0, gold0, [0])
            # Where the window is clamped several vectors predict the same pixels and the full-pel step may settle elsewhere; in
            # the interior macro block of 48 x 48 the planted vector is the one found, at no cost.  Its blocks see all nine
            # offsets over the launches.
            if n == 9 and four:
                assert ms["s4"][4] == 0 and np.array_equal(ms["bvx"][4], vx[4]) and np.array_equal(ms["bvy"][4], vy[4])
                seen |= set(zip(vx[4].tolist(), vy[4].tolist()))
            elif n == 9:
                assert (st["smv"][4], st["mvx"][4], st["mvy"][4]) == (0, vx[4, 0], vy[4, 0])
    if n == 9:
        assert seen == {(2 * full[0] + a, 2 * full[1] + b) for a in (-1, 0, 1) for b in (-1, 0, 1)}, seen


TIES = ["flat", "two", ("x", 2, (2, 0)), ("y", 2, (0, 2)), ("x", 2, (1, 0)), ("x", 4, (6, -9)), ("x", 8, (-13, 4)), ("y", 2, (0, -1)), ("y", 4, (8, 5)), ("y", 8, (-2, -14)),
        ("xy", 2, (1, 1)), ("xy", 4, (3, -2)), ("xy", 8, (-7, 9))]
_tie_waves = {}


@pytest.mark.parametrize("kind", TIES, ids=lambda k: k if isinstance(k, str) else "%s%d_%d_%d" % (k[:2] + k[2]))
def test_ties(hip, kind):
    """Content full of equal SADs: the key (SAD, |mv|, raster index) decides, across lanes, waves and the half-pel neighbourhood.
    Period 2 moved by one whole pixel ties the candidates on either side at equal |mv| (the raster index decides), by half a pixel
    the two half-pel neighbours."""
    src0, prev0 = R.tie_content(kind, (48, 48), 3)
    gold0 = R.tie_content(kind, (48, 48), 4)[1]
    st, ms = check_search(src0, prev0, gold0, [0, 25])
    full, half, bci = R.tie_counts(src0, prev0)
    assert (full > 1).any(), "no macro block with a full-pel tie"
    if kind == "flat" or (kind != "two" and kind[1] == 2 and (kind[2][0] | kind[2][1]) & 1):
        assert (half > 1).any(), "no macro block with a half-pel tie"
    _tie_waves[str(kind)] = set((bci[full > 1] % 256 >> 6).tolist())


def test_ties_reach_every_wave(hip):
    """(after test_ties) the winners of the tied macro blocks lie in all four waves' candidates, ci % 256 >> 6"""
    if len(_tie_waves) < len(TIES):   # run alone: the reference's side is all this needs
        for kind in TIES:
            src0, prev0 = R.tie_content(kind, (48, 48), 3)
            full, _, bci = R.tie_counts(src0, prev0)
            _tie_waves[str(kind)] = set((bci[full > 1] % 256 >> 6).tolist())
    assert set().union(*_tie_waves.values()) == {0, 1, 2, 3}
    assert len({frozenset(v) for v in _tie_waves.values()}) > 1


def decision_frame(seed=11):
    """96 x 80: macro blocks of every regime -- PREV moved a little with noise on top, GOLD moved, four blocks moving apart, new
    content -- so that every inequality of both rules has macro blocks near its equality."""
    rng = np.random.default_rng(seed)
    H, W = 80, 96
    n = 30
    smooth = lambda seed: np.clip(np.kron(np.random.default_rng(seed).integers(100, 156, (H // 8 + 4, W // 8 + 4)), np.ones((8, 8))) +
                                  np.random.default_rng(seed + 1).integers(-6, 7, (H + 32, W + 32)), 0, 255)[16:16 + H, 16:16 + W].astype(np.uint8)
    prev0, gold0 = smooth(1), smooth(3)
    bv = rng.integers(-9, 10, (n, 4, 2))
    one = rng.integers(-12, 13, (n, 1, 2))
    regime = np.arange(n) % 5
    bv = np.where((regime == 2)[:, None, None], bv, one)
    bv[(regime == 3) & (np.arange(n) % 2 == 0)] = 0   # (GOLD where it stands: GOLDEN_NOMV)
    from_prev = R.predicted(prev0, bv[:, :, 0], bv[:, :, 1])
    from_gold = R.predicted(gold0, bv[:, :, 0], bv[:, :, 1])
    y, x = np.mgrid[0:H, 0:W]
    reg = regime[(y // 16) * (W // 16) + x // 16]
    amp = np.array([0, 2, 3, 2, 0])[reg]
    src0 = np.where(reg == 3, from_gold, from_prev) + rng.integers(-1, 2, (H, W)) * amp
    src0 = np.where(reg == 4, smooth(seed + 9) // 2 + 60 + rng.integers(-3, 4, (H, W)), src0)
    return np.clip(src0, 0, 255).astype(np.int64), prev0, gold0


def cover(margin_fn, nineq):
    """The fewest lambdas (greedily) at which every inequality stands at -1, 0 and +1 in some macro block, from the candidates the
    statistics give: -> (lambdas, the (inequality, difference) pairs they reach)."""
    reach = {}
    for lam in range(0, 3000):
        for i, m in enumerate(margin_fn(lam)):
            for d in (-1, 0, 1):
                if (m == d).any():
                    reach.setdefault(lam, set()).add((i, d))
    need = {(i, d) for i in range(nineq) for d in (-1, 0, 1)}
    lams, got = [], set()
    while got != need and reach:
        lam = max(reach, key=lambda l: len(reach[l] - got))
        if not reach[lam] - got:
            break
        got |= reach.pop(lam)
        lams.append(lam)
    return lams, got


def test_decision_at_equality(hip):
    """lambda from the reference's statistics: every inequality of the five-mode rule and of the eight-mode cascade is met with its
    sides equal, one apart either way; and lambda 0 and a lambda above every SAD."""
    src0, prev0, gold0 = decision_frame()
    st = R.search(src0, prev0)
    ms = MR.search_all(src0, prev0, gold0)
    l5, got5 = cover(lambda lam: R.margins5(st, lam), 2)
    l8, got8 = cover(lambda lam: MR.decide(ms, lam)["margins"], 5)
    assert got5 == {(i, d) for i in range(2) for d in (-1, 0, 1)}, got5
    assert got8 == {(i, d) for i in range(5) for d in (-1, 0, 1)}, got8
    big = int(max(ms[k].max() for k in ("s0", "smv", "s4", "g0", "gmv", "si"))) + 1
    lams = sorted(set(l5 + l8 + [0, big]))
    check_search(src0, prev0, gold0, lams, st=st, ms=ms)
    modes = set()
    for lam in lams:
        modes |= set(MR.decide(ms, lam)["pix"].tolist())
    assert modes == {R.NOMV, R.INTRA, R.MV, R.GOLDEN_NOMV, R.GOLDEN_MV, R.MV_FOUR}, modes
    assert (MR.decide(ms, big)["pix"] == R.NOMV).all()


@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_picture_region_with_odd_offsets(hip, fmt):
    """64 x 48 with the picture region (1, 2, 61, 45): picture-sized source planes, the frame outside it the picture's clamped edge;
    the search and then the whole stage over its words."""
    from tests import enc_ref
    fw, fh, pic = 64, 48, (1, 2, 61, 45)
    rng = np.random.default_rng(21 + fmt)
    planes = enc_ref.picture("natural", fw, fh, fmt, pic, picture_size=True, seed=5)
    assert planes[0].shape == (45, 61)
    src = R.frame_src(planes, fw, fh, fmt, pic)
    geo = geometry(fw, fh, fmt)
    prev = [np.clip(np.roll(s, (2, -3), (0, 1)) + rng.integers(-6, 7, s.shape), 0, 255).astype(np.uint8) for s in src]
    gold = [np.clip(np.roll(s, (-1, 4), (0, 1)) + rng.integers(-6, 7, s.shape), 0, 255).astype(np.uint8) for s in src]
    tab = tables("qi63")
    for lam in (0, 12):
        got = run((fw, fh), fmt, SEARCH | DECIDE | CODE, 2, src=planes, pic=pic, prev=prev, lam=lam, dequant=tab, from_stats=True)
        st = R.search(src[0], prev[0])
        same(got["stats"], st["words"], "k_rate_me")
        d5 = R.decide5(st, lam)
        same(got["words"], d5["words"], "k_enc_me")
        same(got["from_stats"], d5["words"], "k_enc_mb_modes")
        ref = R.code(geo, src, prev, None, d5["pix"], d5["mv"], None, tab, 2)
        for k in ("levels", "dcq", "cmap", "dcr"):
            same(got[k], ref[k], "five modes: " + k)
        got = run((fw, fh), fmt, DECIDE | CODE, 3, src=planes, pic=pic, prev=prev, gold=gold, lam=lam, dequant=tab)
        d8 = R.decide8(MR.search_all(src[0], prev[0], gold[0]), lam)
        same(got["words"], d8["words"], "k_enc_me_all")
        ref = R.code(geo, src, prev, gold, d8["pix"], d8["mv"], d8["bmv"], tab, 3)
        for k in ("levels", "dcq", "cmap", "dcr"):
            same(got[k], ref[k], "eight modes: " + k)


# ---- P. prediction and quantiser --------------------------------------------------------------------------------------------------
V15 = np.array([-31, -30, -17, -16, -15, -2, -1, 0, 1, 2, 15, 16, 17, 30, 31])


@functools.lru_cache(None)
def noise_planes(fw, fh, fmt, seed):
    rng = np.random.default_rng(seed)
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in [(fh, fw), (fh >> vd, fw >> hd), (fh >> vd, fw >> hd)])


def check_code(frame, fmt, pix, mv, bmv, tab, classes, src=None, prev=None, gold=None):
    """Stage (c) over given words against the reference.  -> the reference's dict"""
    fw, fh = frame
    geo = geometry(fw, fh, fmt)
    src = list(noise_planes(fw, fh, fmt, 1)) if src is None else src
    prev = list(noise_planes(fw, fh, fmt, 2)) if prev is None else prev
    gold = list(noise_planes(fw, fh, fmt, 3)) if gold is None else gold
    bm = np.zeros((len(pix), 4, 2), np.int64) if bmv is None else bmv
    if classes == 2:
        words = R.pack_words5(pix, mv[:, 0], mv[:, 1])
    else:
        words = R.pack_words8(pix, mv, bm, np.zeros((len(pix), 2), np.int64))
    got = run(frame, fmt, CODE, classes, src=top(src), prev=prev, gold=gold if classes == 3 else None, dequant=tables(tab), words=words)
    ref = R.code(geo, [s.astype(np.int64) for s in src], prev, gold if classes == 3 else None, pix, mv, bmv, tables(tab), classes)
    for k in ("levels", "dcq", "cmap", "dcr"):
        same(got[k], ref[k], k)
    same(got["words"], words.reshape(got["words"].shape), "the words (an input)")
    return ref


@pytest.mark.parametrize("tab", ["qi63", "flat1"])
@pytest.mark.parametrize("arrangement", [0, 1])
@pytest.mark.parametrize("how", ["mv5", "mv8", "golden_mv"])
@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
def test_single_vector(hip, fmt, how, arrangement, tab):
    """240 x 240, every macro block its own vector of V15 x V15: whole, half and (decimated chroma) quarter-pel offsets of both
    signs, reads that leave the frame by up to 16 pixels on each side of each plane; the second arrangement mirrors the first."""
    i, j = np.divmod(np.arange(225), 15)
    mv = np.stack([V15[14 - j], V15[14 - i]] if arrangement else [V15[j], V15[i]], 1)
    pix = np.full(225, R.GOLDEN_MV if how == "golden_mv" else R.MV)
    ref = check_code((240, 240), fmt, pix, mv, None, tab, 2 if how == "mv5" else 3)
    geo = geometry(240, 240, fmt)
    for p, g in enumerate(geo.planes):   # both signs at all four edges of every plane
        nh, nv, o = g["nhfrags"], g["nvfrags"], g["froffset"]
        vx, vy = ref["fvx"][o:o + nh * nv].reshape(nv, nh), ref["fvy"][o:o + nh * nv].reshape(nv, nh)
        seen = {(vx[:, 0] < 0).any(), (vx[:, -1] > 0).any(), (vy[0] < 0).any(), (vy[-1] > 0).any()}
        assert seen == {bool(1 - arrangement)}, (p, seen)


@pytest.mark.parametrize("tab", ["qi63", "flat1"])
@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
def test_all_pixel_modes_mixed(hip, fmt, tab):
    """One frame that mixes the six pixel modes, random vectors in [-31, 31]; and its five-mode half through the five-mode kernel."""
    rng = np.random.default_rng(31 + fmt)
    n = 15 * 15
    pix = rng.choice([R.NOMV, R.INTRA, R.MV, R.GOLDEN_NOMV, R.GOLDEN_MV, R.MV_FOUR], n)
    mv = np.where(np.isin(pix, [R.MV, R.GOLDEN_MV])[:, None], rng.integers(-31, 32, (n, 2)), 0)
    bmv = np.where((pix == R.MV_FOUR)[:, None, None], rng.integers(-31, 32, (n, 4, 2)), 0)
    ref = check_code((240, 240), fmt, pix, mv, bmv, tab, 3)
    assert {1, 2, 3} <= set(np.unique(ref["cmap"]))
    pix5 = rng.choice([R.NOMV, R.INTRA, R.MV], n)
    check_code((240, 240), fmt, pix5, np.where((pix5 == R.MV)[:, None], rng.integers(-31, 32, (n, 2)), 0), None, tab, 2)


@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
def test_mv_four_chroma_vectors(hip, fmt):
    """MV_FOUR everywhere with random block vectors: the chroma vector is the rounded average of four (4:2:0) or two (4:2:2), ties
    away from zero -- asserted to occur at negative and at positive sums -- and the block's own in 4:4:4."""
    rng = np.random.default_rng(41 + fmt)
    n = 8 * 8
    bmv = rng.integers(-31, 32, (n, 4, 2))
    bmv[0], bmv[1], bmv[2], bmv[3] = -31, [[-31, -31], [-31, -31], [-31, -31], [-29, -29]], 31, [[-31, -30], [-30, -31], [31, 30], [30, 31]]
    if fmt == 0:
        sums = bmv.sum(1)
        tie = np.abs(sums) % 4 == 2
    elif fmt == 2:
        sums = np.concatenate([bmv[:, 0] + bmv[:, 1], bmv[:, 2] + bmv[:, 3]])
        tie = np.abs(sums) % 2 == 1
    if fmt != 3:
        for c in range(2):
            assert (tie[:, c] & (sums[:, c] < 0)).any() and (tie[:, c] & (sums[:, c] > 0)).any()
        assert sums.min() == (-124 if fmt == 0 else -62) and sums.max() == -sums.min()
    ref = check_code((128, 128), fmt, np.full(n, R.MV_FOUR), np.zeros((n, 2), np.int64), bmv, "flat1", 3)
    if fmt == 0:   # the reference rounds them away from zero
        o = geometry(128, 128, 0).froff[1]
        assert np.array_equal(ref["fvx"][o:o + n], np.sign(sums[:, 0]) * ((np.abs(sums[:, 0]) + 2) >> 2))


def single_index_blocks(tab, plane, qti=1):
    """For every zig-zag index z an 8 x 8 residual whose only non-zero level under table (qti, plane) stands at z, found with the
    oracle's transform and quantiser: {z: residual [8, 8]} (an index no amplitude reaches is absent)."""
    import oracle
    from tests.enc_ref import ZIGZAG
    t = tables(tab)[qti, plane].astype(np.uint16)
    c = lambda k: np.sqrt(0.5) if k == 0 else 1.0
    x = np.arange(8)
    out = {}
    for z in range(64):
        v, u = divmod(int(ZIGZAG[z]), 8)
        basis = c(u) * c(v) / 4 * np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))
        for amp in range(2, 400):
            for sign in (1, -1):
                res = np.round(sign * amp * basis).astype(np.int16)
                if np.abs(res).max() > 100:
                    continue
                lev, _ = oracle.quantize_batch(oracle.fdct8x8_batch(res.reshape(1, 64)), t)
                nz = np.flatnonzero(lev[0])
                if len(nz) == 1 and nz[0] == z:
                    out[z] = res
                    break
            if z in out:
                break
    return out


@pytest.mark.parametrize("fmt,plane", [(0, 0), (3, 2)], ids=["420-luma", "444-cr"])
def test_nomv_coded_flag(hip, fmt, plane):
    """NOMV everywhere in a 64 x 64 frame: the other planes' source equals PREV (uncoded blocks), and `plane`'s 64 blocks carry a
    residual whose only non-zero level stands at one zig-zag index -- each of the 64 the oracle's quantiser lets a block reach --
    so each lane's share of the coded flag's OR is the only one set once."""
    blocks = single_index_blocks("qi63", plane)
    assert {0, 1, 63} <= set(blocks) and all(any(8 * k + i in blocks for i in range(8)) for k in range(8)), sorted(blocks)
    assert len(blocks) == 64, "indices out of the quantiser's reach: %r" % sorted(set(range(64)) - set(blocks))
    geo = geometry(64, 64, fmt)
    prev = [np.full(s.shape, 128, np.uint8) + (np.arange(s.shape[1]) % 7).astype(np.uint8) for s in noise_planes(64, 64, fmt, 0)]
    src = [a.astype(np.int64) for a in prev]
    for z in sorted(blocks):
        by, bx = divmod((z * 5) % 64, 8)   # index z in block 5 z mod 64: neighbours in memory are not neighbours in index
        src[plane][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] += blocks[z]
    src = [np.clip(a, 0, 255).astype(np.uint8) for a in src]
    for classes in (2, 3):
        ref = check_code((64, 64), fmt, np.zeros(16, np.int64), np.zeros((16, 2), np.int64), None, "qi63", classes, src=src, prev=prev)
        o = geo.froff[plane]
        cm = ref["cmap"]
        assert (cm[o:o + 64] == 2).all() and cm.sum() == 128, "the planted blocks, and only they, are coded"
        lev = ref["lev"][o:o + 64]
        assert ((lev != 0).sum(1) == 1).all() and {int(np.flatnonzero(l)[0]) for l in lev} == set(range(64))


# ---- D. the DC alone --------------------------------------------------------------------------------------------------------------
GEOS, MAPS, dc_case = R.GEOS, R.MAPS, R.dc_case


@pytest.mark.parametrize("classes", [2, 3])
@pytest.mark.parametrize("geo_name,kind", [(g, k) for g in GEOS for k in MAPS if k != "far" or g == "1536x1024"])
def test_dc_alone(hip, geo_name, kind, classes):
    """Stage (d) against dc_residuals.  From the reference's trace: on the large geometry the dense and half maps meet all sixteen
    neighbour masks in every class and each of the three 128-range corrections of masks 7 and 15; the far and edges maps put the
    fall-back where their comments say (far needs more than 257 chunks: the large geometry only)."""
    geo, cm, dcq = dc_case(geo_name, kind, classes)
    assert dcq.min() == -2000 and dcq.max() == 2000
    trace = []
    ref = MR.dc_residuals(geo, dcq.astype(np.int64)[:, None], cm != 0, cm.astype(np.int64), classes, trace=trace).astype(np.int16)
    assert np.array_equal(ref, R.dc(geo, cm, dcq, classes))
    big = geo_name == "1536x1024"
    if big and kind in ("dense", "half"):
        for c in range(1, classes + 1):
            assert {m for _, k, m, _ in trace if k == c} == set(range(16)), c
        assert {(m, fix) for _, _, m, fix in trace if fix} == {(m, f) for m in (7, 15) for f in (1, 2, 3)}
    if kind == "far":
        at = {f: m for f, _, m, _ in trace}
        assert at[270 * 256 + 17] == 0 and ref[270 * 256 + 17] == dcq[270 * 256 + 17]                   # cut at the plane's start
        assert at[285 * 256 + 77] == 0 and ref[285 * 256 + 77] == dcq[285 * 256 + 77] - dcq[258 * 256 + 3]   # from chunk 258
        assert ref[285 * 256 + 79] == dcq[285 * 256 + 79] - dcq[285 * 256 + 77]
    if kind == "edges":
        at = {f: m for f, _, m, _ in trace}
        for p in (1, 2):
            o = geo.froff[p]
            if geo.planes[p]["nfrags"] > 2:
                assert at[o + 2] == 0 and ref[o + 2] == dcq[o + 2], "the previous plane's last fragment must not be used"
            if geo.planes[p]["nfrags"] > 3 and classes == 3:
                assert at[o + 3] == 0 and ref[o + 3] == dcq[o + 3]
        if big:
            assert at[768 + 5] == 0 and ref[768 + 5] == dcq[768 + 5] - dcq[767]      # the last fragment of chunk 2
            assert at[256 + 6] == 0 and ref[256 + 6] == dcq[256 + 6] - dcq[256]      # the first fragment of chunk 1
    got = run(GEOS[geo_name][:2], GEOS[geo_name][2], DC, classes, cmap=cm, dcq=dcq)
    same(got["dcr"], ref, "dcr")
    same(got["cmap"], cm, "cmap (an input)")
    same(got["dcq"], dcq, "dcq (an input)")


def test_dc_plane_first_fragment(hip):
    """The cut `last > froff[p]`: the plane's first fragment itself is a fall-back (last = froff + 1), the fragment before it is not
    (last = froff) -- in the two chroma planes of 272 x 16, and with the classes swapped."""
    geo = geometry(272, 16, 0)
    for classes in (2, 3):
        for swap in (False, True):
            cm = np.zeros(geo.nfrags, np.uint8)
            a, b = (2, 1) if swap else (1, 2)
            for p in (1, 2):
                o = geo.froff[p]
                cm[[o - 1, o + 5]] = a     # the previous plane's last, then isolated: predicts 0
                cm[[o, o + 9]] = b         # the plane's first, then isolated: predicts it
            dcq = np.random.default_rng(3).integers(-2000, 2001, geo.nfrags).astype(np.int16)
            ref = R.dc(geo, cm, dcq, classes)
            for p in (1, 2):
                o = geo.froff[p]
                assert ref[o + 5] == dcq[o + 5] and ref[o + 9] == dcq[o + 9] - dcq[o] and ref[o] == dcq[o]
            same(run((272, 16), 0, DC, classes, cmap=cm, dcq=dcq)["dcr"], ref, "dcr")


def test_dc_refuses_a_class_beyond_its_count(hip):
    geo = geometry(16, 16, 0)
    cm = np.array([1, 2, 3, 0, 0, 0], np.uint8)
    run((16, 16), 0, DC, 2, cmap=cm, dcq=np.zeros(geo.nfrags, np.int16), expect_rc=-10)
