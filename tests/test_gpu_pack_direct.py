"""The five kernels of the device packetiser (theora_amd/csrc/thip_encode_pack.h) driven directly, through thip_enc_pack_tokens, at
every span, run and bit edge: synthetic token streams (tests/packref.py's builders) fix what a picture would otherwise have to
land on -- where a span, a tile or a piece of 4095 ends, where the first token of an index above 0 stands, how many tiles share a
32-bit word, how long a code is, which table wins.  Every case asserts that the bytes and the record equal packref.pack exactly, and
that the output tensor beyond the packet's last word still holds the pattern it was filled with.

A span is S = ceil(ceil(T / groups) / 256) * 256 tokens, a tile 256."""
import numpy as np
import pytest

from tests import packref as P

pytestmark = pytest.mark.gpu

_FILL = None


def span(T, groups):
    return ((T + groups - 1) // groups + 255) // 256 * 256


def check(hip, words, ll, tables, groups, phase, cap=None):
    """One call of the entry against packref.pack.  cap: cap_bytes (default the least that fits: need + 4).  Returns the record."""
    import torch
    from theora_amd.encoder import pack_tokens
    global _FILL
    if _FILL is None:
        _FILL = ((torch.arange(1 << 18, dtype=torch.int32, device="cuda") * 7 + 3) & 0xFF).to(torch.uint8)
    codes, lens = tables
    data, rec = P.pack(words, ll, codes, lens, phase)
    need = rec["bytes"]
    cap = need + 4 if cap is None else cap
    size = max(cap, need + 4) + 61   # one allocation, larger than cap_bytes
    assert size <= len(_FILL)
    out = _FILL[:size].clone()
    d_words = torch.from_numpy(np.concatenate([words, np.zeros(1, np.uint32)]).view(np.int32)).cuda()
    torch.cuda.synchronize()
    rc, got = pack_tokens(d_words.data_ptr(), ll, codes, lens, groups, phase, out.data_ptr(), cap)
    assert got == rec, (got, rec)
    if need + 4 > cap:
        assert rc == 2
        assert torch.equal(out, _FILL[:size])
        return rec
    assert rc == 0
    keep = (need + 3) // 4 * 4
    assert torch.equal(out[keep:], _FILL[keep:size])
    mine = out[:need].cpu().numpy().tobytes()
    if mine != data:
        bad = [i for i in range(need) if mine[i] != data[i]]
        raise AssertionError("%d of %d bytes differ, first at %d: %02x for %02x (T %d, groups %d, phase %d)" %
                             (len(bad), need, bad[0], mine[bad[0]], data[bad[0]], len(words), groups, phase))
    return rec


def mixed(T, first_ac, seed, density=0.5, tokens=None):
    rng = np.random.default_rng(seed)
    ll = P.lists(T, first_ac, rng)
    return P.stream(ll, P.mask(T, density, rng), rng, tokens), ll


_tables = {}


def tab(kind, seed=1, want=None):
    key = (kind, seed, None if want is None else tuple(want))
    if key not in _tables:
        _tables[key] = P.tables(kind, np.random.default_rng(seed), want)
    return _tables[key]


# ---- sizes x groups ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ac", [False, True], ids=["dc-only", "with-ac"])
@pytest.mark.parametrize("groups", [1, 2, 3, 4, 512])
@pytest.mark.parametrize("T", [0, 1, 255, 256, 257, 511, 512, 513, 768])
def test_sizes_and_groups(hip, T, groups, ac):
    """Every size around a tile and a span edge with one to more groups than tiles (the last spans empty); T = 0 is the 16 bits of
    table indices."""
    words, ll = mixed(T, T // 3 if ac else None, 100 + T)
    for kind in ("default", "len32"):
        rec = check(hip, words, ll, tab(kind), groups, 3)
        assert (rec["merged_ac"] > 0) == (ac and T > 0)
        if T == 0:
            assert (rec["bits"], rec["bytes"]) == (0, 3)


# ---- phase ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", range(8))
@pytest.mark.parametrize("what", ["mixed", "empty", "all-eob"])
def test_every_phase(hip, what, phase):
    T = 0 if what == "empty" else 300
    words, ll = mixed(T, T // 2, 7, density=1.0 if what == "all-eob" else 0.4)
    for groups in (1, 2):
        check(hip, words, ll, tab("default"), groups, phase)


# ---- the first token of an index above 0 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("T,at", [(T, at) for T in (258, 768) for at in (0, 1, 255, 256, 257, 511, 512, T - 1, None) if at is None or at < T])
def test_first_ac_token_anywhere(hip, T, at, groups):
    """The AC table indices stand in front of the first token of an index above 0: with no index-0 token at all, in any lane of any
    tile, as a span's first (256 of 258 in 2 groups, 256 and 512 of 768 in 3) and last token (255; 257 of 258), as the stream's last
    token, and at the very end when there is no such token.  No EOBs, so the stream index is the merged one."""
    words, ll = mixed(T, at, 31 * T + (at or 0), density=0.0)
    rec = check(hip, words, ll, tab("default"), groups, 5)
    assert rec["merged_ac"] == (0 if at is None else T - at)
    words, ll = mixed(T, at, 31 * T + (at or 0) + 1, density=0.5)
    check(hip, words, ll, tab("len32"), groups, 2)


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("at", [255, 256, 257])
@pytest.mark.parametrize("to_end", [False, True])
def test_run_from_index_0_into_index_1(hip, at, groups, to_end):
    """A piece that starts in an index-0 list and runs into index 1 counts as DC, and the AC indices follow it -- in front of the next
    token, or, when the run goes on to the stream's end, at the end."""
    T = 768
    rng = np.random.default_rng(at)
    ll = P.lists(T, at, rng)
    m = P.run_mask(T, at - 3, T - at + 3 if to_end else 10, rng, density=0.0)
    rec = check(hip, P.stream(ll, m, rng), ll, tab("default"), groups, 1)
    assert rec["merged_ac"] == (0 if to_end else T - at - 7) and rec["merged"] == at - 3 + 1 + rec["merged_ac"]


# ---- run lengths ------------------------------------------------------------------------------------------------------------------
RUNS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 4094, 4095, 4096, 8190, 8191, 3 * 4095 + 1)


def _placements(L):
    """(T, groups, start): the run at the stream's first and last word, and starting or ending one before, at and one after a tile
    edge that is no span edge and a span edge."""
    T, groups = (((L + 700) // 256 + 1) * 256, 2) if L < 4000 else (((L + 1500) // 256 + 1) * 256, 8)
    S = span(T, groups)
    tile_lo, tile_hi = 256, (T - 1) // 256 * 256
    if tile_hi % S == 0:
        tile_hi -= 256
    span_lo, span_hi = S, (T - 1) // S * S
    assert tile_lo % S and tile_hi % S and 0 < span_lo <= span_hi < T and min(tile_hi, span_hi) - 1 - L >= 0
    starts = {0, T - L}
    for edge in (tile_lo, span_lo):
        starts |= {edge + d for d in (-1, 0, 1)}              # the run's first word one before, at, one after the edge's first word
    for edge in (tile_hi, span_hi):
        starts |= {edge + d - L for d in (-1, 0, 1)}          # its last word: the edge's last word is edge - 1
    return [(T, groups, s) for s in sorted(starts) if 0 <= s and s + L <= T]


@pytest.mark.parametrize("L", RUNS)
def test_run_lengths_at_tile_and_span_edges(hip, L):
    for T, groups, start in _placements(L):
        rng = np.random.default_rng(L * 31 + start)
        ll = P.lists(T, T // 2, rng)
        words = P.stream(ll, P.run_mask(T, start, L, rng, density=0.3), rng)
        rec = check(hip, words, ll, tab("default"), groups, (start + L) % 8)
        assert rec["merged"] < T
        check(hip, words, ll, tab("default"), 1, 0)


def test_piece_ends_on_a_span_edge(hip):
    """S = 4096 with 3 groups of 12 288 tokens; the run starts at 1, so its first piece's last word, 4095, is span 0's last word, and
    the second piece's, 8190, lies one before span 1's."""
    T, L = 12288, 8190 + 40
    assert span(T, 3) == 4096
    rng = np.random.default_rng(2)
    ll = P.lists(T, 6000, rng)
    words = P.stream(ll, P.run_mask(T, 1, L, rng), rng)
    check(hip, words, ll, tab("default"), 3, 4)
    words = P.stream(ll, P.run_mask(T, 2, L, rng), rng)   # ... and with both one further
    check(hip, words, ll, tab("default"), 3, 4)


@pytest.mark.parametrize("groups", [1, 4, 512])
def test_whole_stream_one_run(hip, groups):
    T = 2 * 4095 + 5
    ll = P.lists(T, 5000, np.random.default_rng(0))
    rec = check(hip, P.stream(ll, np.ones(T, bool), np.random.default_rng(0)), ll, tab("default"), groups, 4)
    assert (rec["merged"], rec["merged_ac"]) == (3, 1)


@pytest.mark.parametrize("groups", [1, 4, 7])
def test_pieces_in_different_lists(hip, groups):
    """Three pieces of 4095 and one of 1: the first starts in luma at index 0, the second in chroma in Huffman group 1, the third there
    too, the last in the other chroma plane in group 4 -- with tables in which every class has another best table and all codes differ."""
    ll = P.lists_from({(0, 0): 4000, (3, 2): 4300, (20, 0): 200, (40, 1): 4000, (50, 0): 300})
    rng = np.random.default_rng(9)
    T, L = 12800, 3 * 4095 + 1
    words = P.stream(ll, P.run_mask(T, 5, L, rng, density=0.4), rng, tokens=(P.LUMA_TOKENS, P.CHROMA_TOKENS))
    zp = P.stream_lists(ll)
    assert [tuple(zp[5 + 4095 * k]) for k in range(4)] == [(0, 0), (3, 2), (3, 2), (40, 1)]
    want = [(3,), (0,), (12,), (6,)]   # (no chroma token at index 0 outside the run: table 0)
    rec = check(hip, words, ll, tab("pick", 4, want), groups, 6)
    assert rec["huff"] == [w[0] for w in want]


# ---- sparse and dense tiles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 5, 12, 512])
@pytest.mark.parametrize("what", ["runs-of-256", "isolated"])
def test_sparse_tiles_share_words(hip, what, groups):
    """Codes of one bit.  Runs of 256 EOBs between single value tokens: 13 + 1 bits a tile, so two or three consecutive tiles share
    each 32-bit word of the packet -- with 12 groups every tile is a work group of its own.  Isolated: runs of 300 to 700, so
    some tiles emit nothing."""
    T = 12 * 256
    rng = np.random.default_rng(3)
    ll = P.lists(T, 1500, rng)
    m = np.ones(T, bool)
    if what == "runs-of-256":
        m[256::257] = False
    else:
        m[np.cumsum(rng.integers(300, 700, 4))] = False
    words = P.stream(ll, m, rng, tokens=((9, 10, 11, 12),) * 2)
    for phase in (0, 5):
        rec = check(hip, words, ll, tab("len1"), groups, phase)
        assert rec["bits"] < 13 * 24


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("phase", range(8))
@pytest.mark.parametrize("T", [256, 512])
def test_dense_tiles(hip, T, phase, groups):
    """The tile buffer's worst reachable case: every lane the value token of 10 extra bits with a code of 32 bits, 42 bits a lane
    (with the AC indices in one of them: 256 x 42 + 8 + 8 + 7 + 31 bits at most, kPackBufWords' comment); and its opposite, one bit
    a lane."""
    for first_ac in (None, 100):
        words, ll = mixed(T, first_ac, T + phase, density=0.0, tokens=((22,),) * 2)
        rec = check(hip, words, ll, tab("len32"), groups, phase)
        assert rec["bits"] == 42 * T
        words, ll = mixed(T, first_ac, T + phase, density=0.0, tokens=((9, 10, 11, 12),) * 2)
        assert check(hip, words, ll, tab("len1"), groups, phase)["bits"] == T


# ---- table choice -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [[(0,), (7,), (15,), (9,)], [(15,), (9,), (7,), (0,)]])
def test_each_class_picks_its_own_table(hip, want):
    words, ll = mixed(700, 300, 12, density=0.3, tokens=(P.LUMA_TOKENS, P.CHROMA_TOKENS))
    assert check(hip, words, ll, tab("pick", 6, want), 3, 2)["huff"] == [w[0] for w in want]


@pytest.mark.parametrize("cls", range(4))
def test_tie_goes_to_the_lower_table(hip, cls):
    want = [(2,), (13,), (6,), (10,)]
    want[cls] = (5, 11)
    words, ll = mixed(700, 300, 13 + cls, density=0.3, tokens=(P.LUMA_TOKENS, P.CHROMA_TOKENS))
    assert check(hip, words, ll, tab("pick", 7, want), 2, 7)["huff"] == [w[0] for w in want]


# ---- capacity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 5, 300, 1000])
def test_capacity_rule(hip, T):
    """need + 4 bytes: written.  One byte less: refused with the record filled and not a byte of the tensor touched."""
    words, ll = mixed(T, T // 2, 70 + T)
    need = P.pack(words, ll, *tab("default"), 3)[1]["bytes"]
    for cap in (need + 4, need + 3, need, 4, 0, need + 1000):
        check(hip, words, ll, tab("default"), 2, 3, cap=cap)


# ---- random crosses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", range(8))
def test_random_crosses(hip, batch):
    """25 cases a batch, 200 in all: T up to 2 000 x groups x phase x EOB density x table kind."""
    rng = np.random.default_rng(5000 + batch)
    for k in range(25):
        T = int(rng.integers(0, 2001))
        groups = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 16, 512]))
        kind = ("default", "len32", "len1", "ties", "pick")[(batch * 25 + k) % 5]
        want = [tuple(int(t) for t in rng.choice(16, 1)) for _ in range(4)] if kind == "pick" else None
        tokens = None if kind in ("default", "len32", "len1") else (P.LUMA_TOKENS, P.CHROMA_TOKENS)
        ll = P.lists(T, int(rng.integers(0, T + 1)), rng)
        words = P.stream(ll, P.mask(T, rng.uniform(0.05, 0.98), rng), rng, tokens)
        check(hip, words, ll, P.tables(kind, rng, want), groups, int(rng.integers(0, 8)))
