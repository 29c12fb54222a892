"""tests/packref.py without a GPU: the reference of the device packetiser against itself (unpack(pack(x)) == x), against the
restatement of the encoder that is already pinned to the reference codec (enc_ref.encode_frame), and against what can be said of a
packet by hand; and the refusals of thip_enc_pack_tokens, which come before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import enc_ref
from tests import packref as P

RUNS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 4094, 4095, 4096, 8190, 8191, 3 * 4095 + 1)


def _edge_streams():
    """name -> (words, list_len): what the builders make for the edges the GPU module drives, at sizes a round trip takes no time for."""
    out = {}
    rng = np.random.default_rng(11)
    out["empty"] = (np.zeros(0, np.uint32), P.lists(0, None, rng))
    for T in (1, 255, 256, 257, 513):
        for fa in (None, 0, 1, T - 1):
            if fa is not None and not 0 <= fa < T:
                continue
            ll = P.lists(T, fa, rng)
            out["T%d-ac%s" % (T, fa)] = (P.stream(ll, P.mask(T, 0.5, rng), rng), ll)
    ll = P.lists(300, 100, rng)
    out["all-eob"] = (P.stream(ll, np.ones(300, bool), rng), ll)
    out["no-eob"] = (P.stream(ll, np.zeros(300, bool), rng), ll)
    for L in RUNS:
        T = L + 40
        for start in (0, 17, T - L):
            ll = P.lists(T, T // 3, rng)
            out["run%d-at%d" % (L, start)] = (P.stream(ll, P.run_mask(T, start, L, rng), rng), ll)
    # a run from an index-0 list into index 1 and beyond; pieces whose first words lie in different planes and Huffman groups
    ll = P.lists_from({(0, 0): 50, (0, 1): 20, (0, 2): 20, (1, 0): 30, (6, 1): 40})
    out["run-dc-into-ac"] = (P.stream(ll, P.run_mask(160, 60, 70, rng), rng), ll)
    ll = P.lists_from({(0, 0): 4000, (0, 1): 200, (3, 2): 4000, (20, 0): 300, (40, 1): 4000})
    out["pieces-across-lists"] = (P.stream(ll, P.run_mask(12500, 5, 3 * 4095 + 1, rng), rng), ll)
    return out


EDGES = _edge_streams()


def _round_trip(words, ll, phase):
    codes, lens = P.tables("default")
    data, rec = P.pack(words, ll, codes, lens, phase)
    back, hti, nbits = P.unpack(data, phase, codes, lens, ll)
    assert np.array_equal(back, words)
    assert hti == rec["huff"] and nbits == phase + 16 + rec["bits"] and len(data) == rec["bytes"] == (nbits + 7) >> 3
    return rec


@pytest.mark.parametrize("name", sorted(EDGES))
def test_round_trip_edges(name):
    words, ll = EDGES[name]
    for phase in (0, 3, 7):
        _round_trip(words, ll, phase)


@pytest.mark.parametrize("seed", range(36))
def test_round_trip_random(seed):
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(1, 1500))
    ll = P.lists(T, int(rng.integers(0, T + 1)), rng)
    words = P.stream(ll, P.mask(T, rng.uniform(0.05, 0.98), rng), rng)
    _round_trip(words, ll, int(rng.integers(0, 8)))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
_setup = None


def _setup_params():
    global _setup
    if _setup is None:
        from theora_amd.encoder import Encoder
        e = Encoder(64, 48, 0, 32)
        _setup = enc_ref.SetupParams(e.header_packets()[2])
        e.close()
    return _setup


@pytest.mark.parametrize("kind,w,h,fmt,qi", [("flat", 48, 32, 0, 20), ("noise", 48, 32, 0, 40), ("natural", 64, 48, 0, 30),
                                               ("noise", 32, 32, 3, 63), ("natural", 48, 32, 3, 10), ("flat", 32, 16, 3, 0),
                                               ("flat", 640, 480, 0, 32)])
def test_restatement_packet_is_header_plus_pack(kind, w, h, fmt, qi):
    """enc_ref.encode_frame's packet is its 12 header bits (0, 0, qi, 0, 000) followed by pack() of its own words at phase 4.  The
    flat VGA frame is one run of 7200 EOBs: 4095 in luma, then a piece that begins in luma and ends in the last chroma list."""
    if kind == "natural":
        frame = enc_ref.picture(kind, w, h, fmt, (0, 0, w, h), seed=w + qi)
    else:   # (flat at 128 is all EOBs; noise is dense)
        frame = [np.full(s, 128, np.uint8) if kind == "flat" else enc_ref.content("noise", s, 5) for s in enc_ref.plane_shapes(w, h, fmt)]
    ref = enc_ref.encode_frame(frame, w, h, fmt, (0, 0, w, h), qi, _setup_params())
    codes, lens = P.tables("default")
    data, rec = P.pack(ref["words"], ref["list_len"], codes, lens, 4)
    assert (rec["tokens"], rec["merged"], rec["huff"]) == (ref["tokens"], ref["tokens_merged"], ref["huff"])
    assert data[0] >> 4 == 0
    assert bytes([qi]) + data == ref["packet"]
    if w == 640:
        assert (rec["tokens"], rec["merged"]) == (7200, 2)


# ---- the record -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGES))
def test_record_invariants(name):
    words, ll = EDGES[name]
    rng = np.random.default_rng(5)
    for kind in ("default", "len32", "len1", "ties"):
        codes, lens = P.tables(kind, rng)
        data, rec = P.pack(words, ll, codes, lens, 5)
        merged = P.merge(words, ll)
        assert rec["merged"] == len(merged) <= rec["tokens"] == len(words)
        runs = [P.eob_run(t, x) for _, _, t, x in merged if t <= 6]
        assert all(1 <= r <= 4095 for r in runs) and sum(runs) == int(((words & 31) == 0).sum())
        hti, bits = rec["huff"], 0
        for z, p, t, _ in merged:
            bits += int(lens[16 * P.huff_group(z) + hti[(2 if z else 0) + int(p > 0)]][t]) + P.EXTRA_BITS[t]
        assert bits == rec["bits"] and len(data) == (5 + 16 + bits + 7) >> 3 and data[0] >> 3 == 0


@pytest.mark.parametrize("L", RUNS)
def test_run_pieces(L):
    """A run of L is pieces of 4095 from its start and the rest; each piece belongs to the list of its first EOB."""
    rng = np.random.default_rng(L)
    T = L + 3
    ll = P.lists_from({(0, 0): 2 + min(L, 100), (0, 2): T - 2 - min(L, 100)}) if L < 4000 else \
        P.lists_from({(0, 0): 1000, (0, 1): 3000, (2, 0): 50, (9, 2): T - 4050})
    m = np.zeros(T, bool)
    m[2:2 + L] = True
    merged = P.merge(P.stream(ll, m, rng), ll)
    zp = P.stream_lists(ll)
    want = [(2 + 4095 * k, min(4095, L - 4095 * k)) for k in range((L + 4094) // 4095)]
    got = [(z, p, P.eob_run(t, x)) for z, p, t, x in merged if t <= 6]
    assert got == [(int(zp[at][0]), int(zp[at][1]), n) for at, n in want]
    assert len(merged) == len(want) + 3 and [tok <= 6 for _, _, tok, _ in merged] == [False, False] + [True] * len(want) + [False]


@pytest.mark.parametrize("want", [[(0,), (7,), (15,), (9,)], [(15,), (0,), (3,), (3,)], [(4,), (4,), (12,), (1,)]])
def test_table_built_for_a_histogram_is_chosen(want):
    rng = np.random.default_rng(sum(w[0] for w in want))
    codes, lens = P.tables("pick", rng, want)
    ll = P.lists(600, 250, rng)
    words = P.stream(ll, P.mask(600, 0.3, rng), rng, tokens=(P.LUMA_TOKENS, P.CHROMA_TOKENS))
    assert P.pack(words, ll, codes, lens, 0)[1]["huff"] == [w[0] for w in want]


@pytest.mark.parametrize("cls", range(4))
def test_tie_goes_to_the_lower_index(cls):
    rng = np.random.default_rng(40 + cls)
    want = [(2,), (13,), (6,), (10,)]
    want[cls] = (5, 11)
    codes, lens = P.tables("pick", rng, want)
    ll = P.lists(500, 200, rng)
    words = P.stream(ll, P.mask(500, 0.2, rng), rng, tokens=(P.LUMA_TOKENS, P.CHROMA_TOKENS))
    rec = P.pack(words, ll, codes, lens, 0)[1]
    assert rec["huff"] == [w[0] for w in want]
    # and the tie is one: with table 11's lengths a bit longer the choice is the same, a bit shorter it is 11
    hgs = range(1, 5) if cls >> 1 else range(1)
    alphabet = list(P.CHROMA_TOKENS if cls & 1 else P.LUMA_TOKENS)
    for d, t in ((1, 5), (-1, 11)):
        l2 = lens.astype(np.int64)
        for hg in hgs:
            l2[16 * hg + 11, alphabet] += d
        assert P.choose_tables(P.merge(words, ll), l2)[cls] == t


def test_all_tables_alike_choose_table_0():
    rng = np.random.default_rng(3)
    ll = P.lists(100, 40, rng)
    words = P.stream(ll, P.mask(100, 0.4, rng), rng)
    for kind in ("len32", "len1"):
        codes, lens = P.tables(kind, rng)
        assert P.pack(words, ll, codes, lens, 2)[1]["huff"] == [0, 0, 0, 0]
    data, rec = P.pack(np.zeros(0, np.uint32), P.lists(0, None, rng), codes, lens, 6)
    assert (data, rec["bits"], rec["bytes"]) == (b"\0\0\0", 0, 3)   # T = 0: the 16 bits of table indices at the phase


# ---- the entry's refusals ---------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_without_a_device():
    """NULL pointers, groups, phase, lengths, the list sum and a misaligned packet: refused before anything touches a device (the
    device addresses here are made up)."""
    from theora_amd import _lib
    from theora_amd.encoder import pack_tokens
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "theora_hip.h")).read()
    assert "#define THIP_ENC_PACK_NOFIT %d\n" % _lib.ENC_PACK_NOFIT in hdr and C.sizeof(_lib.EncPackResult) == 48
    rng = np.random.default_rng(0)
    codes, lens = P.tables("len1", rng)
    ll = P.lists(100, 50, rng)
    good = dict(words_ptr=0x1000, list_len=ll, codes=codes, lens=lens, groups=1, phase=0, packet_ptr=0x2000, cap_bytes=4096)

    def rc(**kw):
        return pack_tokens(**dict(good, **kw))[0]
    for name in ("words_ptr", "list_len", "codes", "lens", "packet_ptr"):
        assert rc(**{name: None}) == _lib.EFAULT, name
    L = _lib.load()
    assert L.thip_enc_pack_tokens(0x1000, ll.astype(np.uint32).ctypes.data, codes.ctypes.data, lens.ctypes.data, 1, 0, 0x2000, 4096,
                                  None) == _lib.EFAULT
    for g in (0, -1, _lib.ENC_PACK_MAX_GROUPS + 1, 1 << 20):
        assert rc(groups=g) == _lib.EINVAL, g
    for ph in (-1, 8, 64):
        assert rc(phase=ph) == _lib.EINVAL, ph
    for bad in (0, 33, 255):
        for h, t in ((0, 0), (79, 31), (37, 6)):
            l2 = lens.copy()
            l2[h][t] = bad
            assert rc(lens=l2) == _lib.EINVAL, (bad, h, t)
    big = np.zeros((64, 3), np.int64)
    big[5][1], big[63][2] = (1 << 31) - 1, 1
    assert rc(list_len=big) == _lib.EINVAL
    big[:] = (1 << 32) - 1   # (a sum that does not fit 32 bits either)
    assert rc(list_len=big) == _lib.EINVAL
    for off in (1, 2, 3):
        assert rc(packet_ptr=0x2000 + off) == _lib.EINVAL
