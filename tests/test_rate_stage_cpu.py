"""tests/rate_stage_ref.py against something that is not itself -- its token counting against a scalar loop over
enc_ref.block_tokens, its DC prediction against enc_ref.dc_predict and a scalar spec 7.8; the probe's precondition on the setup's
tables; the grid rule of thip_enc_rate_groups and the bound a histogram bin rests on; the largest coefficient the transform gives;
and the refusals of thip_enc_rate_stage, which come before any device is touched.  No GPU."""
import functools

import numpy as np
import pytest

import oracle
from tests import enc_ref
from tests import rate_stage_ref as R


@functools.lru_cache(None)
def setup():
    from theora_amd.encoder import Encoder
    e = Encoder(16, 16, 0, 63)
    s = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    return s


# ---- the token counting ---------------------------------------------------------------------------------------------------------
def scalar_hist(vals, chroma):
    hist = np.zeros((2, 5, 32), np.int64)
    for v, cc in zip(vals, chroma):
        for tok in enc_ref.block_tokens(v):
            hist[int(cc), enc_ref.huff_group(tok[0]), 0 if tok[1] == "EOB" else tok[1]] += 1
    return hist


def test_token_hist_equals_a_scalar_loop_on_the_planted_edges():
    vals, what = R.edge_blocks()
    n = len(vals)
    for chroma in (np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 3 == 1):
        assert np.array_equal(R.token_hist(vals, chroma), scalar_hist(vals, chroma))
    part = np.arange(n) % 5
    split = R.token_hist(vals, np.zeros(n, bool), part, 5)
    for k in range(5):
        assert np.array_equal(split[k], scalar_hist(vals[part == k], np.zeros((part == k).sum(), bool)))
    # the edges are reached: each block's tokens are what its description says
    for v, (kind, s, gap, a) in zip(vals, what):
        toks = [(t[0], 0 if t[1] == "EOB" else t[1]) for t in enc_ref.block_tokens(v)]
        if kind == "one":
            want = [(s, 9 if a > 0 else 10)] if gap == 0 else [(s, 22 + gap if gap <= 5 else 28 if gap <= 9 else 29)] if gap <= 17 else \
                [(s, 8), (s + gap, 9 if a > 0 else 10)]
        elif kind == "two":
            vt = {2: 11, -2: 12, 3: 13, -3: 13}[a]
            want = [(s, vt)] if gap == 0 else [(s, 30 if gap == 1 else 31)] if gap <= 3 else [(s, 7), (s + gap, vt)]
        elif kind == "run":
            want = [(s, 7 if gap <= 8 else 8), (s + gap, 15)]
        elif kind == "level":
            aa = abs(a)
            want = [(s, (11 if a > 0 else 12) if aa == 2 else 10 + aa if aa <= 6 else 17 if aa <= 8 else 18 if aa <= 12 else 19 if aa <= 20
                     else 20 if aa <= 36 else 21 if aa <= 68 else 22)]
        else:
            continue
        for w in want:
            assert w in toks, (kind, s, gap, a, toks)
    ends = {k: [t for t in enc_ref.block_tokens(v)] for v, k in zip(vals, what) if k[0] in ("end", "empty", "dc")}
    assert all(t[-1][1] != "EOB" for k, t in ends.items() if k[:2] == ("end", 63))       # a value at index 63: no EOB
    assert all(t[-1] == (63, "EOB") for k, t in ends.items() if k[:2] == ("end", 62))
    assert ends[("empty", 0, 0, 0)] == [(0, "EOB")] and ends[("dc", 0, 0, -3)][-1] == (1, "EOB")


def test_token_hist_equals_a_scalar_loop_on_noise():
    rng = np.random.default_rng(1)
    vals = rng.integers(-3, 4, (300, 64)) * (rng.random((300, 64)) < 0.3)
    vals[::7] *= 40
    chroma = rng.random(300) < 0.5
    assert np.array_equal(R.token_hist(vals, chroma), scalar_hist(vals, chroma))


# ---- the DC prediction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nv", [(1, 1), (2, 1), (1, 3), (7, 5), (12, 9)])
def test_dc_pred_masked_equals_enc_ref_with_everything_coded(nh, nv):
    rng = np.random.default_rng(nh * 16 + nv)
    for scale in (3, 200, 2000):   # (2000: the outlier rule of masks 7 and 15 fires)
        dc = rng.integers(-scale, scale + 1, nh * nv)
        avail = R.neighbour_avail(np.ones((nv, nh), bool), np.zeros((nv, nh), bool))
        got = dc.reshape(nv, nh) - R.dc_pred_masked(dc.reshape(nv, nh), avail)
        assert np.array_equal(got.reshape(-1), enc_ref.dc_predict(dc, nh, nv))


def test_dc_pred_masked_equals_a_scalar_spec_for_every_mask():
    rng = np.random.default_rng(7)
    nh, nv = 9, 8
    seen, fallback, negative = set(), set(), set()
    for trial in range(40):
        ok = rng.random((nv, nh)) < 0.7
        cl = rng.random((nv, nh)) < 0.5
        dc = rng.integers(-300, 301, (nv, nh)) * rng.choice([1, 1, 9], (nv, nh))
        if trial % 4 == 3:   # a level plane with a few low cells: left and upper agree, the upper-left one is the outlier
            dc = np.where(rng.random((nv, nh)) < 0.15, 50, 200 + rng.integers(-5, 6, (nv, nh)))
            ok[:] = True
            cl[:] = False
        avail = R.neighbour_avail(ok, cl)
        pred = R.dc_pred_masked(dc, avail)
        for fy in range(nv):
            for fx in range(nh):
                m, v = 0, [0, 0, 0, 0]
                for k, (dy, dx) in enumerate(((0, -1), (-1, -1), (-1, 0), (-1, 1))):
                    y, x = fy + dy, fx + dx
                    if y >= 0 and 0 <= x < nh and ok[y, x] and cl[y, x] == cl[fy, fx]:
                        m |= 1 << k
                        v[k] = int(dc[y, x])
                assert m == R.neighbour_mask(avail)[fy, fx]
                want = R.dc_pred_scalar(m, *v)
                assert pred[fy, fx] == want, (m, v, pred[fy, fx], want)
                seen.add(m)
                l, ul, u, ur = v
                num = {5: l + u, 9: 75 * l + 53 * ur, 11: 75 * l + 53 * ur, 13: 75 * l + 53 * ur, 10: ul + ur, 14: 3 * (ul + ur) + 10 * u,
                       7: 29 * (l + u) - 26 * ul, 15: 29 * (l + u) - 26 * ul}.get(m)
                den = {5: 2, 9: 128, 11: 128, 13: 128, 10: 2, 14: 16, 7: 32, 15: 32}.get(m)
                if num is not None and num < 0 and num % den:
                    negative.add(den)   # a negative operand that the division truncates towards zero
                if m in (7, 15):
                    p = abs(num) // 32 * (1 if num >= 0 else -1)
                    fallback.add("u" if abs(p - u) > 128 else "l" if abs(p - l) > 128 else "ul" if abs(p - ul) > 128 else "none")
    assert seen == set(range(16)) and fallback == {"u", "l", "ul", "none"} and negative == {2, 16, 32, 128}


def test_dc_pred_scalar_truncates_towards_zero():
    assert R.dc_pred_scalar(5, -3, 0, 0, 0) == -1 and R.dc_pred_scalar(5, 3, 0, 0, 0) == 1
    assert R.dc_pred_scalar(9, -1, 0, 0, -1) == -1 and R.dc_pred_scalar(9, -1, 0, 0, 0) == 0
    assert R.dc_pred_scalar(14, 0, -1, 0, 0) == 0 and R.dc_pred_scalar(14, 0, -1, -1, -1) == -1
    assert R.dc_pred_scalar(15, 100, 90, 110, 7) == 117     # 3750 / 32, within 128 of all three
    assert R.dc_pred_scalar(15, 200, 0, 200, 7) == 200      # 362 is more than 128 from u: u
    assert R.dc_pred_scalar(7, 0, 0, 300, 0) == 0           # 271 is within 128 of u and more than 128 from l: l
    assert R.dc_pred_scalar(7, 200, 50, 200, 0) == 50       # 321 is within 128 of u and l and more than 128 from ul: ul
    assert R.dc_pred_scalar(7, -1, 0, 0, 0) == 0 and R.dc_pred_scalar(7, -33, 0, 0, 0) == -29   # -29 / 32, -957 / 32


def test_dc_unpredict_inverts_the_residuals():
    geo = R.geometry(48, 32, 0)
    rng = np.random.default_rng(3)
    ok = rng.random(geo.nfrags) < 0.8
    cl = rng.random(geo.nfrags) < 0.5
    resid = rng.integers(-40, 41, geo.nfrags)
    dc = R.dc_unpredict(geo, resid, ok, cl)
    got, _ = R.dc_residuals(geo, dc, ok, cl)
    assert np.array_equal(got[ok], resid[ok])


# ---- the probe's precondition ---------------------------------------------------------------------------------------------------
def test_setup_steps_are_least_at_qi_63():
    """k_rate_dc and k_rate_tok walk only the indices whose coefficient is not zero at qi 63: for every table and index of the
    encoder's setup header the step at qi 63 is the least over q (thip_enc_rate_stage refuses tables of which this is not true)."""
    steps = R.steps_of(setup()).astype(np.int64)
    assert steps.shape == (6, 64, 64) and steps.min() >= 1 and steps.max() <= 32767
    assert np.array_equal(steps[:, 63, :], steps.min(1))
    assert np.array_equal(R.steps_decreasing()[:, 63, :], R.steps_decreasing().min(1))
    assert (np.diff(R.steps_decreasing().astype(np.int64), axis=1) < 0).all()


# ---- the grid rule and the bin bound ----------------------------------------------------------------------------------------------
def blocks_of_busiest_group(n, groups):
    return int(np.bincount(R.group_of(n, groups), minlength=groups).max())


def largest_count_of_a_block():
    """The most one block adds to one bin: a token starts at an index once, a bin is one token of one Huffman group, so at most the
    indices of the largest group -- and a block of +-1 at each of them reaches it."""
    size = np.bincount(R.HG[:64])
    v = np.zeros((1, 64), np.int64)
    v[0, 27:] = 1
    assert R.token_hist(v, np.zeros(1, bool)).max() == size.max()
    rng = np.random.default_rng(0)
    vals = rng.integers(-2, 3, (400, 64))
    for b in vals:
        assert (R.token_hist(b[None], np.zeros(1, bool)).sum(2)[0] <= size).all()   # (all tokens of a group: no more than its indices)
    return int(size.max())


def test_grid_rule_keeps_every_bin_below_16_bits():
    from theora_amd.encoder import rate_groups
    per_block = largest_count_of_a_block()
    assert per_block == 36
    for n in list(range(1, 20001)) + [245759, 245760, 245761, 245762, 1 << 24]:
        g = rate_groups(n)
        assert g >= 1, n
        assert g == max(min(256, -(-n // 16)), -(-n // 960)), n
        rounds = -(-n // 16)
        blocks = 16 * -(-rounds // g)                         # the busiest group's: its 16 waves take a block a round
        if n <= 20000 and n % 37 == 0:
            assert blocks >= blocks_of_busiest_group(n, g) > blocks - 16
        assert blocks <= -(-n // g) + 16 <= 976, (n, g, blocks)
    assert 976 * per_block < 65536 and 1019 * per_block < 65536   # (1019: the most the entry accepts of a caller's count)
    assert rate_groups(0) == -10 and rate_groups(-5) == -10 and rate_groups((1 << 24) + 1) == -10


# ---- the coefficient bound ------------------------------------------------------------------------------------------------------
def test_transform_of_extreme_residuals_stays_in_int16():
    blocks = R.extreme_residuals()
    assert np.abs(blocks).max() == 255 and len(blocks) == 72
    bound = R.coef_bound()
    assert 255 * 8 <= bound < 1 << 15   # (the DC of a flat block alone is 8 * 255)
    print("largest coefficient:", bound)


# ---- the entry's refusals ---------------------------------------------------------------------------------------------------------
A = 0x10000   # a device address nobody reads: every case below is refused before a device is touched
OK_KW = dict(frame=(64, 48), pixel_fmt=0, inter=1, stages=15, pic=(1, 2, 61, 45), groups=0, fixed=28, src=[A + 1] * 3, src_pitch=[63, 33, 33],
             prev=[A] * 3, ref_pitch=[64, 32, 32], steps=np.ones(6 * 64 * 64), lam=np.ones(64), lens=np.ones(80 * 32), stats=A, coef=A,
             qdc=A, coded=A, cls=A, partial=A, est=A)


def _steps(t, q, z, v):
    s = np.full((6, 64, 64), 8)
    s[t, q, z] = v
    return s


REFUSALS = [
    ("no stage", dict(stages=0), -10), ("unknown stage", dict(stages=16), -10), ("negative stages", dict(stages=-1), -10),
    ("inter 2", dict(inter=2), -10), ("inter -1", dict(inter=-1), -10),
    ("width 0", dict(frame=(0, 48)), -10), ("height not a multiple of 16", dict(frame=(64, 40)), -10),
    ("width 2^20", dict(frame=(1 << 20, 48)), -10), ("too many fragments", dict(frame=(65536, 65536), pixel_fmt=3), -10),
    ("format 1", dict(pixel_fmt=1), -10), ("format 4", dict(pixel_fmt=4), -10),
    ("negative groups", dict(groups=-1), -10), ("groups above the rule's maximum", dict(groups=17478), -10),
    ("1024 blocks a group", dict(frame=(256, 128), pixel_fmt=2, pic=None, groups=1, stages=8), -10),
    ("1024 blocks a group of two", dict(frame=(512, 128), pixel_fmt=2, pic=None, groups=2, stages=8), -10),
    ("picture beyond the frame", dict(pic=(4, 2, 61, 45)), -10), ("picture height 0", dict(pic=(1, 2, 61, 0)), -10),
    ("negative pic_x", dict(pic=(-1, 2, 61, 45)), -10),
    ("no source plane", dict(src=[A, None, A]), -1), ("no PREV plane", dict(prev=[None, A, A]), -1),
    ("source pitch below the picture", dict(src_pitch=[60, 33, 33]), -10), ("chroma source pitch below", dict(src_pitch=[63, 30, 33]), -10),
    ("reference pitch below the frame", dict(ref_pitch=[63, 32, 32]), -10), ("reference pitch 2^31", dict(ref_pitch=[1 << 31, 32, 32]), -10),
    ("no stats", dict(stats=None), -1), ("no coef", dict(coef=None), -1), ("no coef for DC", dict(coef=None, stages=2), -1),
    ("no steps", dict(steps=None), -1), ("no qdc", dict(qdc=None, stages=4), -1), ("no lambda", dict(lam=None), -1),
    ("no coded", dict(coded=None, stages=2), -1), ("no cls", dict(cls=None, stages=4), -1),
    ("no partial for TOK", dict(partial=None, stages=4), -1), ("no partial for BITS", dict(partial=None, stages=8), -1),
    ("no lens", dict(lens=None, stages=8), -1), ("no est", dict(est=None, stages=8), -1),
    ("a step of 0", dict(steps=_steps(2, 5, 9, 0)), -10), ("a step of 32768", dict(steps=_steps(0, 63, 0, 32768)), -10),
    ("a step at qi 63 above another's", dict(steps=_steps(4, 63, 17, 9)), -10),
    ("a step below qi 63's", dict(steps=_steps(1, 0, 63, 7)), -10),
    ("negative lambda", dict(lam=np.r_[np.ones(63), -1]), -10), ("lambda too large", dict(lam=np.r_[(1 << 24) + 1, np.ones(63)]), -10),
    ("negative fixed", dict(fixed=-1), -10),
    ("stats misaligned", dict(stats=A + 8), -10), ("coef misaligned", dict(coef=A + 8), -10), ("qdc misaligned", dict(qdc=A + 1), -10),
    ("coded misaligned", dict(coded=A + 4), -10), ("cls misaligned", dict(cls=A + 4), -10), ("partial misaligned", dict(partial=A + 2), -10),
    ("est misaligned", dict(est=A + 4), -10),
]


@pytest.mark.parametrize("what,change,rc", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_entry_refusals(what, change, rc):
    from theora_amd.encoder import rate_stage
    assert rate_stage(**dict(OK_KW, **change)) == rc, what


def test_a_stage_asks_only_for_what_it_reads():
    """Refused for the one thing wrong, with everything another stage would need left out."""
    from theora_amd.encoder import rate_stage
    none = dict(src=None, prev=None, steps=None, lam=None, lens=None, stats=None, coef=None, qdc=None, coded=None, cls=None, partial=None)
    assert rate_stage(**dict(OK_KW, **dict(none, stages=8, est=A + 4, partial=A, lens=np.ones(2560)))) == -10   # BITS: partial, lens, est
    assert rate_stage(**dict(OK_KW, **dict(none, stages=8, inter=0, partial=A, lens=np.ones(2560), est=None))) == -1
    # a key frame's DC and TOK read neither stats, lambda, coded nor cls: the bad step is what is found
    assert rate_stage(**dict(OK_KW, **dict(none, stages=6, inter=0, coef=A, qdc=A, partial=A, steps=_steps(0, 0, 0, 0)))) == -10


def test_entry_takes_a_wrong_table_size_for_the_callers_mistake():
    from theora_amd.encoder import rate_stage
    for k, v in (("steps", np.ones(384)), ("lam", np.ones(63)), ("lens", np.ones(80))):
        with pytest.raises(ValueError):
            rate_stage(**dict(OK_KW, **{k: v}))
