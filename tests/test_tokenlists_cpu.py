"""tests/tokenlists.py against itself, no GPU: the walk of decode.c:1540-1581 over what the packer made gives the frame's levels back,
for every run cap and token form, pixel format, frame type and list shape the GPU tests (tests/test_gpu_token_lists.py) hand to the
kernels, and the tables satisfy what include/theora_hip.h says of them and thip_state_token_lists_append checks."""
import numpy as np
import pytest

import theora_amd
from tests import tokenlists as T
from theora_amd import synth

CAPS = [1, 4095, None]


def check(geom, frame, res, cap, combine):
    """pack -> invariants -> walk == the frame.  Returns (lists, walk)."""
    L = T.pack(geom, frame, eob_cap=cap, combine=combine, dc_residual=res)
    nc = L["ncoded"]
    ntok = L["tokens"].size
    off, ln, carry, arr = (L[k].astype(np.int64) for k in ("list_off", "list_len", "eob_carry", "arrivals"))
    assert (off + ln <= ntok).all() and ln.sum() == ntok            # the lists lie inside the array and make it up
    assert (arr <= np.asarray(nc)[:, None]).all() and (carry <= arr).all()
    assert (arr[:, 0] == nc).all()                                  # every coded fragment is open at index 0
    assert (carry[0, 0] == 0)
    tok = L["tokens"].astype(np.int64)
    eob = (tok & T.TOK_EOB) != 0
    run = (tok & 0xFFFF) | (tok >> 24) << 16
    assert (run[eob] >= 1).all() and (cap is None or (run[eob] <= cap).all())
    assert ((tok[~eob] >> 24) == 0).all()
    if not combine:                                                 # a token is a zero run or a value, never both
        assert (((tok[~eob] >> 16) & 127 == 0) | (tok[~eob] & 0xFFFF == 0)).all()
    W = T.walk(L)
    lv = np.asarray(frame["levels"], np.int16).reshape(-1, 64)
    assert np.array_equal(W["levels"][:, 1:], lv[:, 1:])
    assert np.array_equal(W["levels"][:, 0], np.asarray(res, np.int16))
    assert np.array_equal(L["dc"], lv[:, 0])
    # the counts the walk observes
    assert np.array_equal(W["arrivals"], arr) and np.array_equal(W["used"], ln) and np.array_equal(W["carried"], carry)
    # a fragment arrives once per token it meets: what the lists consume is what arrives
    for p in range(3):
        for z in range(64):
            t = tok[off[p, z]:off[p, z] + ln[p, z]]
            e = (t & T.TOK_EOB) != 0
            inside = arr[p, z] - carry[p, z]                        # arrivals the list's own tokens serve
            cost = np.where(e, (t & 0xFFFF) | (t >> 24) << 16, 1)
            if cost.size == 0:
                assert inside == 0, (p, z)
                continue
            assert cost[:-1].sum() < inside <= cost.sum(), (p, z)   # every token serves an arrival; only the last may reach past the list
            assert e[-1] or cost.sum() == inside, (p, z)
    # last_zzi: the index of the last token met (decode.c:1545)
    Zq = lv[:, synth.FZIG_ZAG].astype(np.int64)
    Zq[:, 0] = res
    nz = Zq != 0
    lastv = np.where(nz.any(1), 63 - np.argmax(nz[:, ::-1], axis=1), -1)
    ends = lastv < 63
    assert np.array_equal(W["last_zzi"][ends], (lastv[ends] + 1).astype(np.uint8))
    if not combine:
        assert (W["last_zzi"][~ends] == 63).all()
    return L, W


@pytest.mark.parametrize("combine", [True, False])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("ftype", [theora_amd.INTRA_FRAME, theora_amd.INTER_FRAME])
@pytest.mark.parametrize("fmt", [theora_amd.PF_420, theora_amd.PF_422, theora_amd.PF_444])
def test_walk_gives_the_levels_back(fmt, ftype, cap, combine):
    geom = synth.Geometry(80, 48, fmt)
    rng = np.random.default_rng(100 * fmt + 10 * ftype + (cap or 7))
    for content in ("mixed", "smooth", "dense"):
        fr = synth.gen_frame(geom, rng, ftype, content)
        check(geom, fr, T.residuals(fr, rng), cap, combine)
        check(geom, fr, T.predicted_residuals(geom, fr), cap, combine)


def base(geom, rng, counts=None, p_ac=0.1):
    fr = synth.gen_frame(geom, rng, theora_amd.INTER_FRAME, dict(synth.CLASSES["mixed"], p_coded=1.0))
    if counts is not None:
        fr = T.with_coded(geom, fr, counts, rng)
    fr = T.sparse(geom, fr, rng, p_ac, big=0.1)
    fr["dc_residual"] = T.residuals(fr, rng)
    return fr


def test_with_coded_and_sparse():
    geom = synth.Geometry(512, 256, theora_amd.PF_420)
    rng = np.random.default_rng(5)
    fr = base(geom, rng, [2047, 33, 500])
    assert fr["ncoded"] == [2047, 33, 500] and fr["coded_fragis"].size == 2580
    assert fr["coded_fragis"].size + fr["uncoded_fragis"].size == geom.nfrags
    assert (fr["refi"][fr["uncoded_fragis"]] == 3).all() and (fr["refi"][fr["coded_fragis"]] < 3).all()
    assert (np.diff(geom.frag_pos[fr["coded_fragis"]]) > 0).all()       # still the coded order
    for k in ("coeffs", "levels", "last_zzi", "dc_quant", "qii"):
        assert len(fr[k]) == 2580
    assert np.array_equal(fr["coeffs"], synth.dequantise(geom, fr))
    L, _ = check(geom, fr, fr["dc_residual"], None, True)
    assert 1.0 < L["tokens"].size / 2580 < 1.6                          # about 1.3 tokens a fragment
    assert (np.abs(fr["levels"].astype(int)) > 127).any()


M_SMALL = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025]
M_RANK = [4095, 4096, 4097, 8193]


@pytest.mark.parametrize("z", [0, 1, 63])
def test_a_list_of_exactly_m_tokens(z):
    rng = np.random.default_rng(60 + z)
    for ms, (w, h, fmt) in ((M_SMALL, (512, 256, theora_amd.PF_444)), (M_RANK, (1024, 576, theora_amd.PF_420))):
        geom = synth.Geometry(w, h, fmt)
        full = base(geom, rng)
        for i, m in enumerate(ms):
            plane = i % 3 if fmt == theora_amd.PF_444 else 0
            fr = full
            if z == 0:
                counts = list(full["ncoded"])
                counts[plane] = m
                fr = T.with_coded(geom, full, counts, rng)
            fr = T.shape_list(geom, fr, plane, z, m, rng)
            for cap in CAPS:
                for combine in (True, False):
                    L, _ = check(geom, fr, fr["dc_residual"], cap, combine)
                    assert L["list_len"][plane][z] == m and L["arrivals"][plane][z] == m, (m, cap, combine)


@pytest.mark.parametrize("share", [32, 64])
def test_list_shape_edges(share):
    geom = synth.Geometry(512, 256, theora_amd.PF_444)
    rng = np.random.default_rng(share)
    frames = T.edge_frames(geom, base(geom, rng, [2048, 2000, 1999]), rng, share)
    assert sorted(frames) == ["carry_minus_1", "ended_at_0", "last_alive", "run_to_plane_end", "run_to_share_end", "value_at_63"]
    for name, fr in frames.items():
        for cap in CAPS:
            for combine in (True, False):
                L, W = check(geom, fr, fr["dc_residual"], cap, combine)
                if name == "ended_at_0":
                    assert (W["last_zzi"] == 0).all() and (L["arrivals"][:, 1:] == 0).all()
                    if cap is None:   # one run for the whole frame: planes 1 and 2 have no token, their arrivals are all carry
                        assert L["tokens"].tolist() == [T.TOK_EOB | 6047]
                        assert (L["list_len"][1:] == 0).all() and np.array_equal(L["eob_carry"][1:], L["arrivals"][1:])
                if name == "last_alive":
                    assert (L["arrivals"][0, 1:] == 1).all()
                if name == "carry_minus_1" and cap is None:
                    assert L["eob_carry"][1][0] == L["arrivals"][1][0] - 1 == 1999
                if name == "run_to_plane_end" and cap is None:
                    assert L["eob_carry"][1][0] == 0 and (L["tokens"][:L["list_len"][0][0]] == (T.TOK_EOB | 40)).any()
                if name == "run_to_share_end" and cap is None:
                    t0 = L["tokens"][:L["list_len"][0][0]]
                    assert (t0 == (T.TOK_EOB | 7)).sum() >= 2
                if name == "value_at_63":
                    assert (W["last_zzi"] == (51 if combine else 63)).sum() > 300


def test_a_run_beyond_16_bits():
    """The whole frame one run of more than 65 535 fragments: bits 24-31 of the token word."""
    geom = synth.Geometry(1024, 1536, theora_amd.PF_444)
    rng = np.random.default_rng(9)
    fr = synth.gen_frame(geom, rng, theora_amd.INTER_FRAME, dict(synth.CLASSES["skip"], p_coded=1.0))
    fr = T.sparse(geom, fr, rng, 0.0)
    res = np.zeros(3 * 24576, np.int16)
    res[-1] = 5
    L, W = check(geom, fr, res, None, True)
    run = 3 * 24576 - 1
    assert run > 65535 and L["tokens"][0] == (T.TOK_EOB | (run & 0xFFFF) | (run >> 16) << 24)
    assert L["eob_carry"][1][0] == 24576 and L["eob_carry"][2][0] == 24575


def test_groups_of_indices_are_pieces_of_the_array():
    geom = synth.Geometry(80, 48, theora_amd.PF_420)
    rng = np.random.default_rng(3)
    fr = synth.gen_frame(geom, rng, theora_amd.INTER_FRAME, "mixed")
    L = T.pack(geom, fr, eob_cap=4095, combine=True, dc_residual=T.residuals(fr, rng))
    got = []
    for z0, z1 in ((0, 3), (3, 10), (10, 28), (28, 48), (48, 64)):
        tok, off = T.group(L, z0, z1)
        for z in range(z0, z1):
            for p in range(3):
                a = int(off[p][z])
                assert np.array_equal(tok[a:a + L["list_len"][p][z]], L["tokens"][L["list_off"][p][z]:][:L["list_len"][p][z]])
        got.append(tok)
    assert np.array_equal(np.concatenate(got), L["tokens"])
