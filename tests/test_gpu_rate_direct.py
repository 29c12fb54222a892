"""The rate probe of th_encode_*'s bitrate mode driven directly, through thip_enc_rate_stage: the transforms (k_rate_fdct_key,
k_rate_fdct_inter), the quantised DCs and the coded / class ballots (k_rate_dc), the persistent token counter (k_rate_tok) and the
bit sums (k_rate_bits), on inputs no picture produces: every token edge at a start index of every Huffman group, every DC neighbour
mask and outlier fallback, coefficients on either side of every quantiser threshold at every q, modes that flip between q and q + 1
on the equality of each inequality, blocks coded from exactly one q upward, grids in which a wave takes one, two and three blocks,
the heaviest load a histogram bin can carry, Huffman tables that tie.

Every comparison is exact equality with tests/rate_stage_ref.py.  Every "this case reaches that edge" is asserted from the reference
inside the test.  The source has an odd pitch and an odd base address, the reference a pitch that is no multiple of four; every
output lies in front of a guard that must come back untouched, and every input a stage only reads must come back as it was."""
import functools

import numpy as np
import pytest

from tests import enc_inter_ref as IR
from tests import enc_rate_ref as RR
from tests import enc_ref
from tests import inter_stage_ref as IS
from tests import rate_stage_ref as R
from tests.enc_ref import ZIGZAG

pytestmark = pytest.mark.gpu

COEF, DC, TOK, BITS = 1, 2, 4, 8
_GUARD = 64
_DT = dict(stats=np.uint32, coef=np.int16, qdc=np.int16, coded=np.uint64, cls=np.uint64, partial=np.uint32, est=np.int64)

geometry = functools.lru_cache(None)(R.geometry)


@functools.lru_cache(None)
def setup():
    from theora_amd.encoder import Encoder
    e = Encoder(16, 16, 0, 63)
    s = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    return s


@functools.lru_cache(None)
def steps(kind):
    return {"real": lambda: R.steps_of(setup()), "flat1": lambda: R.steps_flat(1), "dec": R.steps_decreasing}[kind]()


@functools.lru_cache(None)
def real_lens():
    return R.code_lengths(setup())


def _upload(planes, pad, base):
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


def run(frame, fmt, inter, stages, pic=None, groups=0, fixed=0, src=None, prev=None, steps=None, lam=None, lens=None, stats=None,
        coef=None, qdc=None, coded=None, cls=None, partial=None):
    """One call of the entry.  src: picture-sized planes, rows top first; prev: frame-sized planes in bitstream row order; the rest
    as tests/rate_stage_ref.py shapes them.  -> dict of what the stages wrote (coef [1 or 3, n, 64], qdc [n, 64], coded, cls [n],
    partial [groups, 64, 321], est [64])."""
    import torch
    from theora_amd.encoder import rate_groups, rate_stage
    n, nmbs = geometry(frame[0], frame[1], fmt).nfrags, (frame[0] // 16) * (frame[1] // 16)
    G = groups or rate_groups(n)
    nvar = 3 if inter else 1
    keep, kw = [], {}
    if src is not None:
        k, kw["src"], kw["src_pitch"] = _upload([np.ascontiguousarray(a, np.uint8) for a in src], 1 if src[0].shape[1] % 2 == 0 else 2, 1)
        keep += k
    if prev is not None:
        k, kw["prev"], kw["ref_pitch"] = _upload([np.ascontiguousarray(a, np.uint8) for a in prev], 5, 0)
        keep += k
    sizes = dict(stats=nmbs * 16, coef=nvar * n * 128, qdc=n * 128, coded=n * 8, cls=n * 8, partial=G * 64 * 321 * 4, est=512)
    writes = ({"coef"} if stages & COEF else set()) | ({"qdc"} | ({"coded", "cls"} if inter else set()) if stages & DC else set()) | \
        ({"partial"} if stages & TOK else set()) | ({"est"} if stages & BITS else set())
    given = dict(stats=stats, coef=coef, qdc=qdc, coded=coded, cls=cls, partial=partial)
    bufs, inits = {}, {}
    for name, size in sizes.items():
        init = None if name in writes else given.get(name)
        if name not in writes and init is None:
            continue
        t = torch.full((size + _GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        if init is not None:
            inits[name] = np.ascontiguousarray(init, _DT[name]).view(np.uint8).reshape(-1)
            assert inits[name].size == size, (name, inits[name].size, size)
            t[:size] = torch.from_numpy(inits[name]).cuda()
        bufs[name] = t
        kw[name] = t.data_ptr()
    torch.cuda.synchronize()
    rc = rate_stage(frame, fmt, inter, stages, pic=pic, groups=groups, fixed=fixed, steps=steps, lam=lam, lens=lens, **kw)
    assert rc == 0, rc
    del keep
    shape = dict(coef=(nvar, n, 64), qdc=(n, 64), coded=(n,), cls=(n,), partial=(G, 64, 321), est=(64,))
    res = {}
    for name, t in bufs.items():
        a = t.cpu().numpy()
        assert (a[sizes[name]:] == 0x5A).all(), "%s: written beyond its end" % name
        if name in writes:
            res[name] = a[:sizes[name]].view(_DT[name]).reshape(shape[name])
        else:
            assert np.array_equal(a[:sizes[name]], inits[name]), "%s: an input was written" % name
    return res


def same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.argwhere(got != ref)
        raise AssertionError("%s: %d of %d differ, first at %s: %r for %r" % (what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])],
                                                                             ref[tuple(bad[0])]))


def picture(fw, fh, fmt, pic, fill, seed=0):
    """Picture-sized planes, rows top first: noise, one value, or a checkerboard of 0 and 255."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in enc_ref.plane_shapes(fw, fh, fmt, pic or (0, 0, fw, fh), picture_size=True):
        if fill == "noise":
            out.append(rng.integers(0, 256, (h, w), dtype=np.uint8))
        elif fill == "checker":
            y, x = np.mgrid[0:h, 0:w]
            out.append((((x + y) & 1) * 255).astype(np.uint8))
        else:
            out.append(np.full((h, w), fill, np.uint8))
    return out


def noise_planes(geo, seed, value=None):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (g["height"], g["width"]), dtype=np.uint8) if value is None else np.full((g["height"], g["width"]), value,
                                                                                                       np.uint8) for g in geo.planes]


def sparse_coef(nvar, n, seed, density=0.06, scale=300):
    """[nvar][n][64] int16, natural order: a few coefficients a block, a few large ones."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-scale, scale + 1, (nvar, n, 64)) * (rng.random((nvar, n, 64)) < density)
    c[:, :, 0] = rng.integers(-2000, 2001, (nvar, n))
    return c.astype(np.int16)


def coef_of_levels(vals):
    """Zig-zag values [n, 64] as natural-order coefficients: under the flat tables of step 1 a level is its coefficient."""
    return R.to_natural(np.asarray(vals, np.int16))[None]


def random_words(rng, n, p):
    return R._bits(rng.random((n, 64)) < p)


FRAMES = [(16, 16, 0), (16, 16, 2), (16, 16, 3), (48, 32, 0), (80, 48, 0)]
FRAME_IDS = ["%dx%d-%d" % f for f in FRAMES]


def regions(fw, fh):
    return [None, (3, 1, fw - 5, fh - 3), (5, 7, 1, 1)]   # the frame; odd offsets and odd sizes; one pixel


# ---- COEF ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
def test_coef_key(hip, frame):
    """n = 6, 8 and 12 leave most of a work group empty; at 48 x 32 and 80 x 48 a wave's sixteen blocks span two planes."""
    fw, fh, fmt = frame
    geo = geometry(fw, fh, fmt)
    if fw > 16:
        assert geo.froff[1] % 16 and geo.froff[2] % 16
    for pic in regions(fw, fh):
        for fill in ("noise", 0, 255, "checker"):
            planes = picture(fw, fh, fmt, pic, fill, seed=fw + fmt)
            src = IS.frame_src(planes, fw, fh, fmt, pic or (0, 0, fw, fh))
            got = run((fw, fh), fmt, 0, COEF, pic=pic, src=planes)
            same(got["coef"], R.coef_key(geo, src), "k_rate_fdct_key %r %r" % (pic, fill))


def planted_vectors(nmbs):
    """Launches of vectors [nmbs, 2]: the corners of the range and odd components on every macro block (so on those at each frame
    edge), then a sweep that gives every component every value of -31..31."""
    out = [np.tile(v, (nmbs, 1)) for v in ((31, 31), (-31, -31), (31, -31), (-31, 31), (1, -1), (-1, 1), (0, 0), (30, -29), (-29, 30), (15, -17))]
    if nmbs >= 6:
        for j in range(-(-63 // nmbs)):
            k = j * nmbs + np.arange(nmbs)
            out.append(np.stack([5 * k % 63 - 31, (11 * k + 31) % 63 - 31], 1))
        swept = np.concatenate(out[10:])
        assert set(swept[:, 0]) == set(swept[:, 1]) == set(range(-31, 32))
    return out


@pytest.mark.parametrize("frame", FRAMES + [(48, 32, 2), (48, 32, 3)], ids=FRAME_IDS + ["48x32-2", "48x32-3"])
def test_coef_inter(hip, frame):
    """The three residual sets, the MV one through planted words: every vector component in -31..31, the corners of the range on the
    macro blocks of every frame edge, chroma vectors of every format; then 0 against 255 and 255 against 0."""
    fw, fh, fmt = frame
    geo = geometry(fw, fh, fmt)
    nmbs = (fw // 16) * (fh // 16)
    rng = np.random.default_rng(fw * 3 + fmt)
    prev = noise_planes(geo, fw + fmt + 1)
    for pic in regions(fw, fh):
        planes = picture(fw, fh, fmt, pic, "noise", seed=fw - fmt)
        src = IS.frame_src(planes, fw, fh, fmt, pic or (0, 0, fw, fh))
        for vec in (planted_vectors(nmbs) if pic is None else planted_vectors(nmbs)[:4]):
            stats = R.pack_stats(*rng.integers(0, 70000, (3, nmbs)), vec[:, 0], vec[:, 1])
            got = run((fw, fh), fmt, 1, COEF, pic=pic, src=planes, prev=prev, stats=stats)
            mvx, mvy = R.stats_vectors(stats)
            assert np.array_equal(mvx, vec[:, 0]) and np.array_equal(mvy, vec[:, 1])
            same(got["coef"], R.coef_inter(geo, src, prev, mvx, mvy), "k_rate_fdct_inter %r %r" % (pic, tuple(vec[0])))
    stats = R.pack_stats(*np.zeros((3, nmbs), np.int64), np.full(nmbs, -3), np.full(nmbs, 5))
    for a, b in ((0, 255), (255, 0)):
        planes = picture(fw, fh, fmt, None, a)
        ref = noise_planes(geo, 0, value=b)
        got = run((fw, fh), fmt, 1, COEF, src=planes, prev=ref, stats=stats)
        want = R.coef_inter(geo, IS.frame_src(planes, fw, fh, fmt, (0, 0, fw, fh)), ref, *R.stats_vectors(stats))
        assert np.array_equal(want[1, 0], R._fdct(np.full((1, 64), a - b))[0])   # (the flat residual at the end of its range)
        same(got["coef"], want, "k_rate_fdct_inter %d against %d" % (a, b))


# ---- DC -----------------------------------------------------------------------------------------------------------------------
def threshold_coef(geo, st, seed):
    """[1][n][64]: sparse noise; block k of each plane has a DC on either side of the threshold of q = k mod 64 -- 2|c| in d - 2 .. d + 2
    of its table's step, both signs; the last blocks of each plane hold +- the transform's bound everywhere."""
    n = geo.nfrags
    coef = sparse_coef(1, n, seed)
    bound = R.coef_bound()
    for p, g in enumerate(geo.planes):
        k = np.arange(g["nfrags"])
        d = st[p, k % 64, 0].astype(np.int64)
        c = ((d - 1) // 2, d // 2, (d + 1) // 2, (d + 2) // 2)
        v = (k // 64) % 8
        coef[0, g["froffset"] + k, 0] = np.choose(v % 4, c) * np.where(v >= 4, -1, 1)
        coef[0, g["froffset"] + g["nfrags"] - 2] = bound
        coef[0, g["froffset"] + g["nfrags"] - 1] = -bound
    return coef


@pytest.mark.parametrize("frame,kind", [((384, 112, 3), "dec"), ((384, 112, 3), "real"), ((16, 16, 0), "flat1"), ((48, 48, 0), "dec"),
                                        ((48, 48, 0), "real"), ((16, 16, 2), "dec")])
def test_dc_key(hip, frame, kind):
    """The quantised DC at every q.  Under the decreasing tables each q has coefficients with 2|c| = d - 1, d and d + 1 of both signs;
    coefficients at +- the bound; n mod 4 = 2 (every frame has an even number of blocks) leaves half of the last work group empty."""
    fw, fh, fmt = frame
    geo = geometry(fw, fh, fmt)
    st = steps(kind)
    coef = threshold_coef(geo, st, fw)
    assert geo.nfrags % 4 == (0 if fw == 384 or fmt == 2 else 2)
    if fw == 384 and kind == "dec":
        k = np.arange(512)
        c = np.stack([coef[0, g["froffset"] + k, 0].astype(np.int64) for g in geo.planes])   # [plane][k]
        d = np.stack([st[p, k % 64, 0].astype(np.int64) for p in range(3)])
        for q in range(64):
            for sign in (1, -1):
                # (2|c| = d needs an even step: at each q one of luma and Cb has one)
                assert {-1, 0, 1} <= set((2 * np.abs(c) - d)[(k % 64 == q)[None, :] & (np.sign(c) == sign)]), (q, sign)
        assert np.abs(coef.astype(np.int64)).max() == R.coef_bound()
    got = run((fw, fh), fmt, 0, DC, coef=coef, steps=st)
    same(got["qdc"], R.dc_stage(geo, coef, st, False)[0], "k_rate_dc<false> %s" % kind)


Q0 = 30
LAM = 20 + 3 * np.arange(64)


def inter_scenario(kind):
    """80 x 48, 4:2:0 (n = 90, n mod 4 = 2), lambda 20 + 3 q, one macro block per case (module docstring):
      0..2   Smv + lambda[Q0] - S0 = 0, -1, +1            3..5  NOMV, SI + 4 lambda[Q0] - S0 = -1, 0, +1
      6..8   MV, SI + 4 lambda[Q0] - Smv = -1, 0, +1       9..11 NOMV at every q, its first, second and last luma block coded from
      Q0 upward alone, through index 0, 63 and 20            12 NOMV, all zero       13 MV at every q       14 INTRA at every q"""
    geo = geometry(80, 48, 0)
    st = steps(kind)
    L = int(LAM[Q0])
    big = 10 ** 6
    rows = [(1000, 1000 - L, big), (1000, 999 - L, big), (1000, 1001 - L, big)]
    rows += [(1000, 1000, 1000 - 4 * L + k) for k in (-1, 0, 1)]
    rows += [(50000, 2000, 2000 - 4 * L + k) for k in (-1, 0, 1)]
    rows += [(0, 0, big)] * 4 + [(10 ** 5, 0, big), (10 ** 5, 10 ** 5, 0)]
    s0, smv, si = np.array(rows).T
    rng = np.random.default_rng(11)
    stats = R.pack_stats(s0, smv, si, rng.integers(-31, 32, 15), rng.integers(-31, 32, 15))
    coef = sparse_coef(3, geo.nfrags, 5)
    quiet = np.isin(geo.mb_of, (9, 10, 11, 12))
    coef[:, quiet] = 0
    planted = {}
    nh = geo.planes[0]["nhfrags"]
    for mb, blk, z, sign in ((9, 0, 0, 1), (10, 1, 63, -1), (11, 3, 20, 1)):
        fi = (mb // 5) * 2 * nh + (mb % 5) * 2 + (blk >> 1) * nh + (blk & 1)
        assert geo.mb_of[fi] == mb
        coef[1, fi, ZIGZAG[z]] = sign * -(-int(st[3, Q0, z]) // 2)   # 2|c| = d or d + 1 at Q0: below the step of Q0 - 1
        planted[mb] = fi
    return geo, st, stats, coef, planted


@pytest.mark.parametrize("kind", ["dec", "real"])
def test_dc_inter(hip, kind):
    """Modes that flip between q and q + 1 on the equality of each inequality of rate_mode; NOMV blocks coded from exactly one q
    upward through index 0 alone, index 63 alone and a mid index alone; an all-zero NOMV block: coded and cls bit by bit."""
    geo, st, stats, coef, planted = inter_scenario(kind)
    m = np.array([R.modes_at(stats, LAM[q]) for q in (Q0 - 1, Q0, Q0 + 1)])
    NOMV, INTRA, MV = IR.NOMV, IR.INTRA, IR.MV
    # equality is "not below": the mode at Q0 is the one above it, and one lambda step to either side moves the neighbours
    assert m[:, 0].tolist() == [MV, NOMV, NOMV] and m[:, 1].tolist() == [MV, MV, NOMV] and m[1, 2] == NOMV
    assert m[:, 3].tolist() == [INTRA, INTRA, NOMV] and m[:, 4].tolist() == [INTRA, NOMV, NOMV] and m[1, 5] == NOMV
    assert m[:, 6].tolist() == [INTRA, INTRA, MV] and m[:, 7].tolist() == [INTRA, MV, MV] and m[1, 8] == MV
    qdc, coded, cls = R.dc_stage(geo, coef, st, True, stats, LAM)
    if kind == "dec":
        for mb, fi in planted.items():
            assert int(coded[fi]) == (1 << 64) - (1 << Q0), (mb, hex(int(coded[fi])))
    quiet = np.isin(geo.mb_of, (9, 10, 11, 12))
    quiet[list(planted.values())] = False
    assert (coded[quiet] == 0).all() and (cls[quiet] == np.uint64(2 ** 64 - 1)).all() and quiet.sum() == 4 * 6 - 3
    assert (coded[geo.mb_of == 13] == np.uint64(2 ** 64 - 1)).all() and (cls[geo.mb_of == 14] == 0).all()
    got = run((80, 48), 0, 1, DC, coef=coef, steps=st, lam=LAM, stats=stats)
    same(got["qdc"], qdc, "k_rate_dc<true> qdc")
    same(got["coded"], coded, "k_rate_dc<true> coded")
    same(got["cls"], cls, "k_rate_dc<true> cls")


# ---- TOK ----------------------------------------------------------------------------------------------------------------------
EDGE_FRAME = (384, 112, 3)   # 672 blocks a plane: every planted block in luma and in both chroma planes


def edge_values(geo):
    vals, what = R.edge_blocks()
    assert all(g["nfrags"] >= len(vals) for g in geo.planes)
    out = np.concatenate([vals[np.arange(g["nfrags"]) % len(vals)] for g in geo.planes])
    return out, what


def test_tok_token_edges(hip):
    """Every planted token edge (tests/test_rate_stage_cpu.py holds each block against its description) at a start index of every
    Huffman group, in luma and in chroma, the DC among them through planted qdc: every bin of every partial, the side count zero."""
    fw, fh, fmt = EDGE_FRAME
    geo = geometry(fw, fh, fmt)
    vals, what = edge_values(geo)
    dc = R.dc_unpredict(geo, vals[:, 0])
    assert np.array_equal(R.dc_residuals(geo, dc, np.ones(geo.nfrags, bool), np.zeros(geo.nfrags, bool))[0], vals[:, 0])
    coef = coef_of_levels(vals)
    qdc = np.repeat(dc[:, None], 64, 1).astype(np.int16)
    st = steps("flat1")
    from theora_amd.encoder import rate_groups
    G = rate_groups(geo.nfrags)
    want = R.tok_stage(geo, coef, qdc, None, None, st, False, groups=G)
    tot = want.sum(0)[0, :320].reshape(2, 5, 32)
    used = [0] + list(range(7, 32))
    assert (tot[:, :, used] > 0).all() and (tot[:, :, 1:7] == 0).all()   # every token but the EOB runs, in every group, luma and chroma
    assert (want[:, :, 320] == 0).all()
    got = run((fw, fh), fmt, 0, TOK, coef=coef, qdc=qdc, steps=st)
    same(got["partial"], want, "k_rate_tok<false> token edges")


def test_tok_divergent_lanes(hip):
    """The planted blocks scaled up under the decreasing tables: every q quantises them differently, so the 64 lanes of a wave walk
    different tokens of one block.  DC | TOK: the quantised DCs are the kernel's own."""
    fw, fh, fmt = EDGE_FRAME
    geo = geometry(fw, fh, fmt)
    vals, _ = edge_values(geo)
    coef = coef_of_levels(np.clip(vals * 37, -32000, 32000))
    st = steps("dec")
    from theora_amd.encoder import rate_groups
    qdc = R.dc_stage(geo, coef, st, False)[0]
    want = R.tok_stage(geo, coef, qdc, None, None, st, False, groups=rate_groups(geo.nfrags))
    assert len(np.unique(want.sum(0)[:, :320], axis=0)) >= 48
    got = run((fw, fh), fmt, 0, DC | TOK, coef=coef, steps=st)
    same(got["qdc"], qdc, "k_rate_dc<false>")
    same(got["partial"], want, "k_rate_tok<false> divergent lanes")


GRID = [((16, 16, 0), 1, 1), ((16, 16, 3), 1, 1), ((48, 32, 0), 3, 1), ((384, 256, 3), 256, 2), ((512, 384, 3), 256, 3)]


@pytest.mark.parametrize("frame,groups,rounds", GRID, ids=["%dx%d-%d" % g[0] for g in GRID])
def test_tok_grid(hip, frame, groups, rounds):
    """n below 16 (waves without a block), n no multiple of 16, and frames of which some waves take two and three blocks: the
    persistent loop's step, and a histogram carried over a wave's second and third block."""
    fw, fh, fmt = frame
    geo = geometry(fw, fh, fmt)
    n = geo.nfrags
    from theora_amd.encoder import rate_groups
    assert rate_groups(n) == groups
    per_wave = np.bincount(np.arange(n) % (16 * groups), minlength=16 * groups)
    assert per_wave.max() == rounds and per_wave.min() < rounds and (n >= 16 or per_wave.min() == 0)
    assert fw != 48 or n % 16
    st = steps("real")
    coef = sparse_coef(1, n, n, density=0.03)
    qdc = R.dc_stage(geo, coef, st, False)[0]
    want = R.tok_stage(geo, coef, qdc, None, None, st, False, groups=groups)
    got = run((fw, fh), fmt, 0, TOK, coef=coef, qdc=qdc, steps=st)
    same(got["partial"], want, "k_rate_tok<false> %d blocks" % n)


@pytest.mark.parametrize("groups", [1, 2])
def test_tok_heaviest_bin(hip, groups, capsys):
    """960 blocks in one and in two work groups, every block +-1 at each index from 28 to 63 after a value at 27: each adds 36 to one
    bin, the most a block can (tests/test_rate_stage_cpu.py), and a group's u16 bin carries all its blocks."""
    fw, fh, fmt = 160, 128, 3
    geo = geometry(fw, fh, fmt)
    n = geo.nfrags
    assert n == 960
    vals = np.zeros((n, 64), np.int64)
    vals[:, 27] = 4
    vals[:, 28:] = np.where(np.arange(n) < geo.froff[1], -1, 1)[:, None]
    coef = coef_of_levels(vals)
    qdc = np.zeros((n, 64), np.int16)
    st = steps("flat1")
    want = R.tok_stage(geo, coef, qdc, None, None, st, False, groups=groups)
    heaviest = int(want[:, :, :320].max())
    assert heaviest == 36 * 640 // groups and heaviest < 65536
    with capsys.disabled():
        print("\nlargest bin of a partial, %d group(s): %d" % (groups, heaviest))
    got = run((fw, fh), fmt, 0, TOK, groups=groups, coef=coef, qdc=qdc, steps=st)
    same(got["partial"], want, "k_rate_tok<false> heaviest bin")


def level_plane(geo, rng):
    """Quantised DCs that meet every fallback of the outlier rule: level planes with a few low cells, and wide noise."""
    n = geo.nfrags
    return np.where(rng.random(n) < 0.5, np.where(rng.random(n) < 0.15, 50, 200 + rng.integers(-5, 6, n)), rng.integers(-2500, 2501, n))


@pytest.mark.parametrize("frame", [(96, 64, 3), (48, 32, 0), (96, 64, 2)], ids=["96x64-3", "48x32-0", "96x64-2"])
def test_tok_inter_planted_ballots(hip, frame):
    """Planted qdc, coded and cls, no two q alike: all 16 neighbour masks in every plane, at the left, right and bottom edge, at the
    first block of a chroma plane (whose fi - 1 lies in the plane before); the three outlier fallbacks and negative truncation; the
    side bits of macro blocks with none of their luma blocks coded, each one alone, MV and not."""
    fw, fh, fmt = frame
    geo = geometry(fw, fh, fmt)
    n, nmbs = geo.nfrags, (fw // 16) * (fh // 16)
    rng = np.random.default_rng(fw + fmt)
    coded, cls = random_words(rng, n, 0.65), random_words(rng, n, 0.5)
    nh = geo.planes[0]["nhfrags"]
    one = np.uint64(2 ** 64 - 1)
    coded[[0, 1, nh, nh + 1]] = 0                             # macro block 0: none coded
    for k, alone in enumerate((0, 1, nh, nh + 1)):            # macro blocks 1..4 (5 of the next row at 48 x 32): each block alone
        mb = 1 + k
        o = (mb // (nh // 2)) * 2 * nh + (mb % (nh // 2)) * 2
        coded[[o, o + 1, o + nh, o + nh + 1]] = 0
        coded[o + alone] = one
    for p in (1, 2):                                          # a chroma plane's first block and the block before it: coded, one class
        coded[[geo.froff[p] - 1, geo.froff[p]]] = one
        cls[[geo.froff[p] - 1, geo.froff[p]]] = 0
    qdc = np.stack([level_plane(geo, rng) for _ in range(64)], 1).astype(np.int16)
    s0 = rng.integers(0, 4000, nmbs)
    stats = R.pack_stats(s0, np.maximum(s0 - rng.integers(0, 400, nmbs), 0), rng.integers(0, 4000, nmbs), rng.integers(-31, 32, nmbs),
                         rng.integers(-31, 32, nmbs))
    coef = sparse_coef(3, n, fw)
    st = steps("dec")
    masks, fallbacks, negative = [set(), set(), set()], set(), set()
    for q in range(64):
        mk, fb, ng = R.dc_cases(geo, qdc[:, q], R.bit(coded, q), R.bit(cls, q))
        masks = [a | b for a, b in zip(masks, mk)]
        fallbacks |= fb
        negative |= ng
    if fw == 96:
        assert all(m == set(range(16)) for m in masks), masks
        assert fallbacks == {"u", "l", "ul", "none"} and negative == {2, 16, 32, 128}
    modes = np.array([R.modes_at(stats, LAM[q]) for q in range(64)])   # [q][mb]
    assert all((modes == m).any() for m in (IR.NOMV, IR.INTRA, IR.MV)) and (modes[0] != modes[63]).any()
    assert (modes[:, 1:5] == IR.MV).any() and (modes[:, 1:5] != IR.MV).any()   # (a macro block with one coded block: 15 bits and 3)
    G = 3
    want = R.tok_stage(geo, coef, qdc, coded, cls, st, True, stats, LAM, groups=G)
    side = want.sum(0)[:, 320]
    assert len(set(side.tolist())) > (8 if fw == 96 else 1) and (side % 3 == 0).all() and side.min() > 0
    got = run((fw, fh), fmt, 1, TOK, groups=G, coef=coef, qdc=qdc, coded=coded, cls=cls, steps=st, lam=LAM, stats=stats)
    same(got["partial"], want, "k_rate_tok<true> planted ballots")


@pytest.mark.parametrize("kind", ["dec", "real"])
def test_tok_inter_scenario(hip, kind):
    """DC | TOK over the macro blocks of inter_scenario: blocks that become coded at exactly Q0, modes that flip around Q0, an empty
    block that is nothing at all when uncoded."""
    geo, st, stats, coef, planted = inter_scenario(kind)
    qdc, coded, cls = R.dc_stage(geo, coef, st, True, stats, LAM)
    want = R.tok_stage(geo, coef, qdc, coded, cls, st, True, stats, LAM, groups=6)
    got = run((80, 48), 0, 1, DC | TOK, coef=coef, steps=st, lam=LAM, stats=stats)
    same(got["coded"], coded, "k_rate_dc<true> coded")
    same(got["partial"], want, "k_rate_tok<true> scenario")
    # macro block 12 alone in a frame: no token and no side bit at any q; in a key frame the same blocks are an EOB each
    zero = np.zeros((3, geo.nfrags, 64), np.int16)
    nomv = R.pack_stats(*np.zeros((3, 15), np.int64), np.zeros(15, np.int64), np.zeros(15, np.int64)) + np.array([0, 0, 10 ** 6, 0], np.uint32)
    got = run((80, 48), 0, 1, DC | TOK, coef=zero, steps=st, lam=LAM, stats=nomv)
    assert (got["coded"] == 0).all() and (got["partial"] == 0).all()
    got = run((80, 48), 0, 0, DC | TOK, coef=zero[:1], steps=st)
    want = R.tok_stage(geo, zero[:1], np.zeros((geo.nfrags, 64), np.int16), None, None, st, False, groups=6)
    assert want.sum() == 64 * geo.nfrags and want[:, :, 0].sum() + want[:, :, 160].sum() == 64 * geo.nfrags   # EOBs of group 0
    same(got["partial"], want, "k_rate_tok<false> empty blocks")


# ---- BITS ---------------------------------------------------------------------------------------------------------------------
def tie_tables():
    """Code lengths 10 everywhere but: token 9 costs 1 in DC tables 2 and 5 (a tie), token 10 costs 1 in DC table 7, token 11 costs 1
    in AC table 11 of every group, token 12 costs 1 in AC table 14 of every group."""
    lens = np.full((80, 32), 10, np.int64)
    lens[2, 9] = lens[5, 9] = lens[7, 10] = 1
    for hg in range(1, 5):
        lens[16 * hg + 11, 11] = lens[16 * hg + 14, 12] = 1
    return lens


@pytest.mark.parametrize("groups", [1, 3, 256, 258])
def test_bits(hip, groups):
    """Planted partials: random counts under the setup's lengths; counts and lengths that let each of the four choices be decided by
    a different table, one of them on a tie; empty histograms; the fixed bits of a key and of an inter frame."""
    rng = np.random.default_rng(groups)
    geo = geometry(16, 16, 0)
    part = rng.integers(0, 65536, (groups, 64, 321)) * (rng.random((groups, 64, 321)) < 0.3)
    part[:, :, 320] = rng.integers(0, 5000, (groups, 64))
    for fixed in (R.FIXED_KEY, R.fixed_inter(geo.nfrags), 0):
        got = run((16, 16), 0, int(fixed == R.fixed_inter(geo.nfrags)), BITS, groups=groups, fixed=fixed, partial=part, lens=real_lens())
        same(got["est"], R.bits_stage(part, real_lens(), fixed), "k_rate_bits, fixed %d" % fixed)
    lens = tie_tables()
    tie = np.zeros((groups, 64, 321), np.int64)
    h = tie[:, :, :320].reshape(groups, 64, 2, 5, 32)
    h[:, :, 0, 0, 9] = rng.integers(1, 50, (groups, 64))
    h[:, :, 1, 0, 10] = rng.integers(1, 50, (groups, 64))
    h[:, :, 0, 1:, 11] = rng.integers(1, 50, (groups, 64, 4))
    h[:, :, 1, 1:, 12] = rng.integers(1, 50, (groups, 64, 4))
    costs = R.table_costs(tie.sum(0)[5, :320].reshape(2, 5, 32), lens)
    assert costs.argmin(1).tolist() == [2, 7, 11, 14] and costs[0, 2] == costs[0, 5] and (np.sort(costs, 1)[1:, 0] < np.sort(costs, 1)[1:, 1]).all()
    got = run((16, 16), 0, 0, BITS, groups=groups, fixed=28, partial=tie, lens=lens)
    same(got["est"], R.bits_stage(tie, lens, 28), "k_rate_bits, tables that tie")
    got = run((16, 16), 0, 0, BITS, groups=groups, fixed=28, partial=np.zeros((groups, 64, 321), np.int64), lens=real_lens())
    assert (got["est"] == 28).all()


# ---- the stages composed --------------------------------------------------------------------------------------------------------
def test_composed_key_frame_equals_the_probe_and_the_encoder(hip):
    """COEF | DC | TOK | BITS on a key frame of 4608 blocks with the setup's tables: Probe.key's E[q], and the E[q] an Encoder in bitrate
    mode reports for the same picture."""
    from tests.test_gpu_encoder_rate import _run
    w, h, fmt = 384, 256, 3
    geo = geometry(w, h, fmt)
    assert geo.nfrags == 4608
    frame = enc_ref.picture("natural", w, h, fmt, (0, 0, w, h), seed=9)
    hdr, out = _run(w, h, fmt, [frame], 10 ** 6)
    su = enc_ref.SetupParams(hdr[2])
    assert np.array_equal(R.steps_of(su), steps("real"))
    got = run((w, h), fmt, 0, COEF | DC | TOK | BITS, fixed=R.FIXED_KEY, src=frame, steps=steps("real"), lens=real_lens())
    want = RR.Probe(w, h, fmt, (0, 0, w, h), su).key(frame)
    same(got["est"], want, "E[q] of a key frame")
    assert out[0][2]["probe"] == [int(x) for x in want]


def test_composed_inter_frame_equals_the_probe_and_the_encoder(hip):
    """The same on an inter frame: the reference is the encoder's own reconstruction of the frame before, the words are the search's
    (thip_enc_inter_stage) on the same planes."""
    from tests.test_gpu_encoder_rate import _run
    from tests.test_gpu_inter_direct import SEARCH
    from tests.test_gpu_inter_direct import run as inter_run
    w, h, fmt = 384, 256, 3
    geo = geometry(w, h, fmt)
    frames = IR.sequence("pan", w, h, fmt, 2, seed=5)
    hdr, out = _run(w, h, fmt, frames, 3 * 10 ** 6, inter=True, flags=0, recon=True)
    assert [o[2]["key"] for o in out] == [1, 0]
    su = enc_ref.SetupParams(hdr[2])
    prev = [np.ascontiguousarray(np.flipud(a)) for a in out[0][3]]
    stats = inter_run((w, h), fmt, SEARCH, 2, src=frames[1], prev=prev)["stats"]
    lam = steps("real")[3, :, 1].astype(np.int64)
    got = run((w, h), fmt, 1, COEF | DC | TOK | BITS, fixed=R.fixed_inter(geo.nfrags), src=frames[1], prev=prev, stats=stats,
              steps=steps("real"), lam=lam, lens=real_lens())
    want = RR.Probe(w, h, fmt, (0, 0, w, h), su).inter(frames[1], prev)
    same(got["est"], want, "E[q] of an inter frame")
    assert out[1][2]["probe"] == [int(x) for x in want]
