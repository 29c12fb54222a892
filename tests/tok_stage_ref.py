"""What thip_enc_tok_stage (include/theora_hip.h) must hand out, restated in numpy and Python integers: the tokeniser of th_encode_*
between the quantising kernels and the packetiser.  The token rule is enc_ref.block_tokens (and streamgen's value_token under
it), the DC predictor enc_ref.dc_predict; the words are in the format of theora_amd/csrc/thip_encode.h (token | extra << 5 |
index << 16 | plane << 22, an EOB token 0).

  tokens(geo, classes, levels, dcq / dcr, cmap)   stage TOK: tok [n][65] with ntok [n] (the words that are written), mask [n],
                                                  chunk_cnt [nchunks][3][64], overflow, and `cover`: the branches taken
  scan(chunk_cnt)                                 stage SCAN: chunk_base [nchunks][64], list_len [3][64]
  scatter(tok, mask, chunk_base, list_len)        stage SCATTER: out, and which of its words were written
  restate(...)                                    the three in a row
  stream_words(t)                                 the stream order a second way: tokens()'s tokens sorted by (index, plane, block)

All-zero blocks (one EOB at index 0) never enter a Python loop, so a frame of 65664 blocks of which a few hundred hold levels
is restated in well under a second."""
import functools

import numpy as np

from tests import enc_ref
from tests.enc_inter_ref import Geometry

TOK_WORDS, CHUNK, MAX_LEVEL = 65, 256, 580


@functools.lru_cache(maxsize=None)
def geometry(fw, fh, fmt):
    return Geometry(fw, fh, fmt)


def nchunks(n):
    return (n + CHUNK - 1) // CHUNK


def _tdiv(a, b):
    """C's division (towards zero) on int64 arrays, b > 0."""
    return np.where(a >= 0, a // b, -((-a) // b))


def _plane_residuals(q, nh, nv):
    """enc_ref.dc_predict on one plane, called only on the rows that hold a DC or lie above one that does (the residual of a
    fragment whose neighbours and own DC are all zero is zero)."""
    q2 = q.reshape(nv, nh)
    live = q2.any(1)
    live[1:] |= live[:-1].copy()
    res = np.zeros((nv, nh), np.int64)
    fy = 0
    while fy < nv:
        if not live[fy]:
            fy += 1
            continue
        end = fy
        while end < nv and live[end]:
            end += 1
        lo = max(fy - 1, 0)   # (the row below is all zero unless fy is 0: as a first row it stands in for itself)
        res[lo:end] = enc_ref.dc_predict(q2[lo:end].reshape(-1), nh, end - lo).reshape(end - lo, nh)
        if lo < fy:
            res[lo] = 0       # (an all-zero row predicted from all-zero rows)
        fy = end
    return res.reshape(-1)


def _dc_cover(q, pred, nh, nv, cover):
    """Which branches of spec 7.8 a key frame's plane takes, from its DCs alone; where the weighted predictor is used, its value
    formed here must be the one enc_ref.dc_predict used."""
    q2, p2 = q.reshape(nv, nh).astype(np.int64), pred.reshape(nv, nh)
    fx, fy = np.meshgrid(np.arange(nh), np.arange(nv))
    m = (fx > 0) * 1 | ((fx > 0) & (fy > 0)) * 2 | (fy > 0) * 4 | ((fy > 0) & (fx + 1 < nh)) * 8
    for v in np.unique(m):
        cover.add(("mask", int(v)))
    w = (m & 7) == 7
    if not w.any():
        return
    ys, xs = np.nonzero(w)
    l, u, ul = q2[ys, xs - 1], q2[ys - 1, xs], q2[ys - 1, xs - 1]
    num = 29 * (l + u) - 26 * ul
    p0 = _tdiv(num, 32)
    fb = np.where(np.abs(p0 - u) > 128, 1, np.where(np.abs(p0 - l) > 128, 2, np.where(np.abs(p0 - ul) > 128, 3, 0)))
    got = np.choose(fb, [p0, u, l, ul])
    assert np.array_equal(got, p2[ys, xs]), "the DC predictor's two statements differ"
    for v in np.unique(fb):
        cover.add(("fallback", ("none", "u", "l", "ul")[int(v)]))
    # where two tests fail at once and their values differ, the order of the tests shows
    fu, fl, ful = np.abs(p0 - u) > 128, np.abs(p0 - l) > 128, np.abs(p0 - ul) > 128
    if (fu & fl & (u != l)).any():
        cover.add(("fallback", "u before l"))
    if (~fu & fl & ful & (l != ul)).any():
        cover.add(("fallback", "l before ul"))
    inexact = num % 32 != 0
    for sign, sel in ((1, num > 0), (-1, num < 0)):
        if (sel & inexact).any():
            cover.add(("div32", sign))


def key_residuals(geo, levels, dcq, cover=None):
    """The DC residual of every block of a key frame, coded order: its own DC is levels[k][0], its predictor is made of dcq."""
    dcq = np.asarray(dcq, np.int64)
    pred = np.zeros(geo.nfrags, np.int64)
    for p, g in enumerate(geo.planes):
        sl = slice(g["froffset"], g["froffset"] + g["nfrags"])
        pred[sl] = dcq[sl] - _plane_residuals(dcq[sl], g["nhfrags"], g["nvfrags"])
        if cover is not None:
            _dc_cover(dcq[sl], pred[sl], g["nhfrags"], g["nvfrags"], cover)
    return np.asarray(levels, np.int64)[:, 0] - pred[geo.coded_order]


def _rule_cover(v, cover):
    """The boundaries of the token rule a block's values touch: (class of the value, zero run before it), the value itself."""
    nz = np.nonzero(v)[0]
    nxt = 0
    for z in nz:
        a = int(v[z])
        aa = abs(a)
        cover.add(("gap", 1 if aa == 1 else 23 if aa <= 3 else 4, int(z) - nxt))
        cover.add(("value", max(min(a, MAX_LEVEL + 1), -MAX_LEVEL - 1)))
        nxt = int(z) + 1


def tokens(geo, classes, levels, dcq=None, dcr=None, cmap=None, want_cover=True):
    """Stage TOK.  levels [n][64] coded order; dcq (classes 0) or dcr and cmap (classes 2, 3) raster."""
    n, order = geo.nfrags, geo.coded_order
    V = np.array(levels, np.int64).reshape(n, 64)
    cover = set()
    if classes == 0:
        V[:, 0] = key_residuals(geo, V, dcq, cover if want_cover else None)
        coded = np.ones(n, bool)
    else:
        V[:, 0] = np.asarray(dcr, np.int64)[order]
        coded = np.asarray(cmap)[order] != 0
    plane = np.asarray(geo.plane_of)[order].astype(np.int64)
    tok = np.zeros((n, TOK_WORDS), np.uint32)
    ntok = np.zeros(n, np.int64)
    mask = np.zeros(n, np.uint64)
    busy = V.any(1) & coded
    empty = coded & ~busy            # one EOB at index 0
    tok[empty, 0] = (plane[empty] << 22).astype(np.uint32)
    ntok[empty] = 1
    mask[empty] = 1
    overflow = 0
    bk, bz, bpos = [np.nonzero(empty)[0]], [np.zeros(int(empty.sum()), np.int64)], [np.zeros(int(empty.sum()), np.int64)]
    for k in np.nonzero(busy)[0]:
        v = V[k]
        overflow += int((np.abs(v) > MAX_LEVEL).sum())
        toks = enc_ref.block_tokens(np.clip(v, -MAX_LEVEL, MAX_LEVEL))   # (beyond 580: the token of 580, 22 with s << 9 | 511)
        p, m = int(plane[k]), 0
        for i, t in enumerate(toks):
            z = t[0]
            tok[k, i] = (z << 16 | p << 22) | (0 if t[1] == "EOB" else t[1] | t[2] << 5)
            m |= 1 << z
            if want_cover:
                cover.add(("tok", 0 if t[1] == "EOB" else t[1]))
        if want_cover:
            _rule_cover(v, cover)
            if toks[-1][1] != "EOB":
                cover.add(("tok", "no-eob"))
            if (np.abs(v) > MAX_LEVEL).any():
                cover.add(("tok", "overflow"))
        ntok[k] = len(toks)
        mask[k] = m
        bk.append(np.full(len(toks), k))
        bz.append(np.array([t[0] for t in toks], np.int64))
        bpos.append(np.arange(len(toks)))
    bk, bz, bpos = np.concatenate(bk), np.concatenate(bz), np.concatenate(bpos)
    if want_cover and empty.any():
        cover.add(("tok", 0))
    cnt = np.zeros((nchunks(n), 3, 64), np.int64)
    np.add.at(cnt, (bk // CHUNK, plane[bk], bz), 1)
    return dict(tok=tok, ntok=ntok, mask=mask, chunk_cnt=cnt.astype(np.uint32), overflow=overflow, cover=cover, block=bk, index=bz,
                pos=bpos, plane=plane, values=V, coded=coded)


def scan(chunk_cnt):
    """Stage SCAN: chunk_base[c][z] = the tokens of index z in the chunks before c, all planes; list_len[p][z]."""
    c = np.asarray(chunk_cnt, np.int64).reshape(-1, 3, 64)
    per = c.sum(1)
    base = np.cumsum(per, 0) - per
    ll = c.sum(0)
    assert per.sum(0).max(initial=0) < 1 << 32   # (the kernel counts in 32 bits)
    return base.astype(np.uint32), ll.astype(np.uint32)


def scatter(tok, mask, chunk_base, list_len):
    """Stage SCATTER on any tok [n][65], mask [n], chunk_base, list_len: (out, of sum(list_len) words; written: which of them a
    block's token went to; clash: whether two tokens went to one word)."""
    tok, mask = np.asarray(tok), np.asarray(mask, np.uint64)
    n = len(mask)
    ll = np.asarray(list_len, np.int64).reshape(3, 64).sum(0)
    start = np.cumsum(ll) - ll
    total = int(ll.sum())
    B = ((mask[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)   # [n][64]
    t = np.cumsum(B, 1) - B                                  # the word of the block that holds its token of index z
    rank = np.cumsum(B, 0) - B
    first = (np.arange(n) // CHUNK) * CHUNK                  # the chunk's first block
    rank -= rank[first]                                      # ... counted from the chunk's start
    pos = start[None, :] + np.asarray(chunk_base, np.int64).reshape(-1, 64)[np.arange(n) // CHUNK] + rank
    ks, zs = np.nonzero(B)
    out = np.zeros(total, np.uint32)
    written = np.zeros(total, bool)
    where = pos[ks, zs]
    assert where.size == 0 or (0 <= where.min() and where.max() < total), "a token's place lies outside the stream"
    out[where] = tok[ks, t[ks, zs]]
    written[where] = True
    return out, written, len(np.unique(where)) != len(where)


def restate(geo, classes, levels, dcq=None, dcr=None, cmap=None, want_cover=True):
    """Every output of the entry with all three stages asked for."""
    r = tokens(geo, classes, levels, dcq, dcr, cmap, want_cover)
    r["chunk_base"], r["list_len"] = scan(r["chunk_cnt"])
    r["out"], written, clash = scatter(r["tok"], r["mask"], r["chunk_base"], r["list_len"])
    assert written.all() and not clash
    return r


def stream_words(t):
    """The words of tokens()'s result in stream order, by sorting alone: index, then plane, then coded order."""
    o = np.lexsort((t["pos"], t["block"], t["plane"][t["block"]], t["index"]))
    return t["tok"][t["block"][o], t["pos"][o]]


# ---- what the tests feed the entry ---------------------------------------------------------------------------------------------------
VALUES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 20, 21, 36, 37, 68, 69, 580)
# (class of the value, zero run in front of it) on both sides of every boundary of the rule
RULE_EDGES = [(1, g) for g in (0, 1, 5, 6, 9, 10, 17, 18)] + [(23, g) for g in (0, 1, 2, 3, 4)] + [(4, g) for g in (0, 1, 8, 9)]


def rule_cases(seed, extra):
    """Blocks of one value behind a zero run, (next, gap, value): the first level +-4 at index next - 1 (none for next 0), the value at
    next + gap.  Every boundary gap of the rule with every value of VALUES and both signs at the earliest and the latest start that
    holds it and a start between; then `extra` seeded draws from the whole grid."""
    rng = np.random.default_rng(seed)
    cases = []
    for gap in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 17, 18, 63):
        for v in VALUES:
            for s in (1, -1):
                for nxt in sorted({0, (63 - gap) // 2, 63 - gap}):
                    cases.append((nxt, gap, s * v))
    for _ in range(extra):
        nxt = int(rng.integers(0, 64))
        cases.append((nxt, int(rng.integers(0, 64 - nxt)), int(rng.choice(VALUES)) * int(rng.choice((1, -1)))))
    return cases


def rule_blocks(cases):
    lv = np.zeros((len(cases), 64), np.int16)
    for i, (nxt, gap, v) in enumerate(cases):
        if nxt:
            lv[i, nxt - 1] = 4 if i & 1 else -4
        lv[i, nxt + gap] = v
    return lv


def shaped_blocks(rng):
    """The block shapes no single value reaches: all 64 levels set (no EOB), index 63 alone, nothing, zeros alternating with
    |a| >= 4 from index 0 and from index 1, every level +-1, a long run into +-1 at 63."""
    out = []
    big = lambda size: (rng.integers(4, 581, size) * rng.choice((1, -1), size)).astype(np.int16)
    for _ in range(3):
        out.append((rng.integers(1, 581, 64) * rng.choice((1, -1), 64)).astype(np.int16))
    for v in (1, -1, 2, -3, 4, -580):
        b = np.zeros(64, np.int16)
        b[63] = v
        out.append(b)
    out.append(np.zeros(64, np.int16))
    for first in (0, 1):
        b = np.zeros(64, np.int16)
        b[first::2] = big(32)
        out.append(b)
    out.append(rng.choice((1, -1), 64).astype(np.int16))
    return np.stack(out)


def dc_plane(nh, nv, rng, kind):
    """A plane of quantised DCs (raster) that takes spec 7.8's branches: "smooth" small steps (the weighted predictor as it is, both
    signs, inexact divisions), "steps" columns and rows of +-400 plateaus (the fallbacks to u, l and ul), "wild" anything in
    +-1000."""
    fx, fy = np.meshgrid(np.arange(nh), np.arange(nv))
    if kind == "smooth":
        q = rng.integers(-3, 4, (nv, nh)) + 5 * np.sign(rng.integers(-1, 2))
    elif kind == "steps":
        # per cell one of the three patterns around it: u apart from l and ul; l apart from u and ul; ul apart
        q = np.where(((fx // 2) + (fy // 2)) % 2 == 0, 400, -400) + rng.integers(-2, 3, (nv, nh))
        q = np.where(rng.random((nv, nh)) < 0.15, q - 150 * np.sign(q), q)   # (as ul: the weighted value leaves it alone)
        q = np.where(rng.random((nv, nh)) < 0.15, rng.integers(-900, 901, (nv, nh)), q)
    else:
        q = rng.integers(-1000, 1001, (nv, nh))
    return q.astype(np.int16).reshape(-1)


def dc_frame(geo, seed):
    """dcq of a whole frame: the three kinds of dc_plane in turn over the planes and the seeds."""
    rng = np.random.default_rng(seed)
    kinds = ("smooth", "steps", "wild")
    return np.concatenate([dc_plane(g["nhfrags"], g["nvfrags"], rng, kinds[(seed + p) % 3]) for p, g in enumerate(geo.planes)])


def sparse_levels(n, blocks, rng):
    """levels [n][64] all zero but for `blocks` (coded-order indices): a few random levels each."""
    lv = np.zeros((n, 64), np.int16)
    for k in blocks:
        m = int(rng.integers(1, 6))
        z = rng.choice(64, m, replace=False)
        lv[k, z] = (rng.integers(1, 40, m) * rng.choice((1, -1), m)).astype(np.int16)
    return lv


def seam_blocks(n, chunks, rng, more=100):
    """Coded-order indices at the starts and ends of `chunks` and at their lanes 63 / 64 / 127 / 128 / 191 / 192, the frame's first
    and last block, and `more` seeded others."""
    ks = {0, n - 1}
    for c in chunks:
        ks |= {c * CHUNK + l for l in (0, 1, 63, 64, 127, 128, 191, 192, 254, 255)}
    ks |= {int(k) for k in rng.integers(0, n, more)}
    return sorted(k for k in ks if 0 <= k < n)
