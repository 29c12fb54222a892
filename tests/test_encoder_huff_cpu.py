"""Custom and trained Huffman codes of th_encode_* (include/theoraenc_hip.h, "Huffman codes") without a GPU: th_encode_alloc,
th_encode_ctl and th_encode_flushheader never touch it, and the trainer is host arithmetic.

Request 0 (refusals, timing, validity -- with the reference encoder's verdict on the same buffers), the setup header's trees from
the codes (against tests/enc_huff_ref.py, the reference decoder's th_decode_headerin and the reference encoder's own header), the
trainer (the library, tests/native/hufftrain_host.cpp under the sanitizers and tests/enc_huff_ref.py, bit for bit), and that
trained codes are lossless in the restatements of the key and inter streams."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_huff_ref as HR
from tests import enc_inter_ref, enc_ref, hufftrain_host, refcmp

W, H = 64, 48
NBYTES = 80 * 32 * 8
E_BIG = C.c_uint8 * NBYTES


def _E():
    from theora_amd import encoder as E
    return E


def _enc(**kw):
    return _E().Encoder(W, H, 0, 32, **kw)


@pytest.fixture(scope="module")
def builtin():
    e = _enc()
    codes = e.huffman_codes()
    e.close()
    return codes


def _set(e, codes, size=None):
    """th_encode_ctl(request 0) with the codes as they are (no check on the Python side) -> the return code."""
    E = _E()
    buf = E._huff_codes_in(codes)
    return e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_SET_HUFFMAN_CODES, C.byref(buf), C.sizeof(buf) if size is None else size)


def _malformed(builtin):
    """One buffer a kind, each wrong in one set only."""
    out = {}
    c = builtin.copy()
    c[17, 4, 1] = 0
    out["a token with nbits 0"] = c
    c = builtin.copy()
    c[3, 9, 1] = 33
    out["nbits 33"] = c
    c = builtin.copy()
    c[40, 1] = c[40, 0]
    out["a duplicate code"] = c
    c = HR.comb_codes()
    c[79, 30], c[79, 31] = (0, 31), (1, 31)   # the two deepest leaves moved under token 0's code "0": the Kraft sum is still 1
    out["a prefix clash"] = c
    c = builtin.copy()
    c[61, 9] = (c[61, 9, 0] << 1, c[61, 9, 1] + 1)   # a leaf one level too deep: its sibling is missing
    out["a Kraft sum below 1"] = c
    c = HR.comb_codes()
    c[0, 31] = ((1 << 30) - 1, 30)   # ... one level too high: it covers token 30's code too
    out["a Kraft sum above 1"] = c
    return out


def _deep_hole():
    """A Kraft sum below 1 at the depth limit: the comb's last leaf as a 32-bit code, its sibling missing.  The reference's
    oc_huff_codes_pack lets this one through (at 32 bits its walk back up the tree shifts its marker bit out of the word and takes
    that for the root) and writes a tree no decoder can read, so only this library's verdict is asserted on it."""
    c = HR.comb_codes()
    c[0, 31] = ((1 << 32) - 1, 32)
    return c


def test_request_0_refusals_and_timing(builtin):
    from theora_amd import _lib as Lm
    E = _E()
    comb = HR.comb_codes(HR.comb_order)
    e = _enc()
    try:
        v = C.c_int(0)
        assert e._L.th_encode_ctl(e._enc, 0, C.byref(v), 4) == Lm.EIMPL
        for size in (0, 4, NBYTES - 1, NBYTES + 8):
            assert _set(e, comb, size) == Lm.EIMPL, size
        assert e._L.th_encode_ctl(e._enc, 0, None, NBYTES) == Lm.EIMPL
        assert np.array_equal(e.huffman_codes(), builtin)
        assert _set(e, comb) == 0
        assert np.array_equal(e.huffman_codes(), comb)
        for kind, bad in dict(_malformed(builtin), deep=_deep_hole()).items():
            assert not HR.valid(bad), kind
            assert _set(e, bad) == Lm.EINVAL, kind
            assert np.array_equal(e.huffman_codes(), comb), kind     # the codes stay as they were
        assert e._L.th_encode_ctl(e._enc, 0, None, 0) == 0           # the built-in codes again
        assert np.array_equal(e.huffman_codes(), builtin)
        assert _set(e, comb) == 0
        hdr = e.header_packets()
        assert _set(e, builtin) == Lm.EINVAL and e._L.th_encode_ctl(e._enc, 0, None, 0) == Lm.EINVAL
        assert np.array_equal(e.huffman_codes(), comb)
        assert np.array_equal(HR.codes_of_setup(enc_ref.SetupParams(hdr[2])), comb)
        buf = E.HuffCodes()
        assert e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_GET_HUFFMAN_CODES, C.byref(buf), NBYTES - 8) == Lm.EINVAL
    finally:
        e.close()
    e = _enc()
    try:   # after the FIRST header packet, not the last
        op, tc = Lm.OggPacket(), Lm.ThComment()
        e._L.th_comment_init(C.byref(tc))
        assert e._L.th_encode_flushheader(e._enc, C.byref(tc), C.byref(op)) == 1
        assert _set(e, comb) == Lm.EINVAL
        assert np.array_equal(e.huffman_codes(), builtin)
    finally:
        e.close()
    with pytest.raises(ValueError):
        _enc(huffman=_malformed(builtin)["a duplicate code"])


def test_python_layer_round_trip(builtin):
    E = _E()
    rot = HR.rotated_codes(builtin)
    assert HR.valid(rot) and not np.array_equal(rot[..., 1], builtin[..., 1])
    dirty = rot.copy()
    dirty[..., 0] |= (np.int64(0xFFFFFFFF) << rot[..., 1]) & 0xFFFFFFFF   # bits above nbits are ignored, and GET masks them
    e = E.Encoder(W, H, 0, 32, huffman=dirty)
    assert np.array_equal(e.huffman_codes(), rot)
    e.set_huffman_codes(None)
    assert np.array_equal(e.huffman_codes(), builtin)
    h = e.token_hist()
    assert h["count"].shape == (5, 2, 32) and not h["count"].any() and h["huff"] == [0] * 4 and h["key"] == 0 and h["device"] == 0
    e.close()


def test_pinned_numbers_stay_free():
    from theora_amd import _lib as Lm
    e = _enc()
    try:
        for req in (0x7216, 0x7217, 0x721A, 0x7220, 0x7221, 0x7224, 0x7299):
            for ctype in (C.c_int, C.c_int64, E_BIG):
                v = ctype()
                assert e._L.th_encode_ctl(e._enc, req, C.byref(v), C.sizeof(v)) == Lm.EIMPL, hex(req)
            assert e._L.th_encode_ctl(e._enc, req, None, 0) == Lm.EIMPL, hex(req)
    finally:
        e.close()


def test_reference_encoder_gives_the_same_verdicts(builtin):
    """The reference's th_encode_ctl on the buffers of the refusal test: the valid ones 0, each malformed one TH_EINVAL."""
    from oracle import ref
    refcmp.need_ref()
    E = _E()
    cases = dict(_malformed(builtin), builtin=builtin, comb=HR.comb_codes(HR.comb_order), rotated=HR.rotated_codes(builtin))
    for kind, codes in cases.items():
        r = ref.RefEncoder(W, H, 0, quality=32)
        buf = E._huff_codes_in(codes)
        rc = r._L.th_encode_ctl(r._enc, 0, C.byref(buf), C.sizeof(buf))
        r.close()
        assert rc == (0 if HR.valid(codes) else ref.TH_EINVAL), kind
        assert (rc == 0) == (kind in ("builtin", "comb", "rotated")), kind


# ---- training pools ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def builtin_setup():
    e = _enc()
    s = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    return s


def _setup_of(codes):
    e = _enc(huffman=codes)
    s = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    return s


def _key_frames():
    return [(kind, q, enc_ref.picture(kind, W, H, 0, seed=3)) for kind in ("natural", "noise", "flat", "gradient") for q in (8, 40, 63)]


def _run_key(setup):
    return [enc_ref.encode_frame(pl, W, H, 0, (0, 0, W, H), q, setup) for _, q, pl in _key_frames()]


def _run_inter(setup, kinds=("pan", "static", "cut"), n=6, qi=32):
    """-> [(packet, histogram, recon)] over the sequences, in order."""
    out = []
    for kind in kinds:
        enc = enc_inter_ref.InterEncoder(W, H, 0, (0, 0, W, H), setup, 64, 6)
        for planes in enc_inter_ref.sequence(kind, W, H, 0, n, seed=5):
            r = enc.frame(planes, qi)
            words = enc_ref.encode_frame(planes, W, H, 0, (0, 0, W, H), qi, setup)["words"] if r["key"] else r.get("words", [])
            out.append((r["packet"], HR.hist_of_words(words) if len(r["packet"]) else np.zeros((5, 2, 32), np.int64), enc.recon))
        enc.close()
    return out


@pytest.fixture(scope="module")
def pools(builtin_setup):
    key = _run_key(builtin_setup)
    inter = _run_inter(builtin_setup)
    key_h = [HR.hist_of_words(r["words"]) for r in key]
    inter_h = [h for _, h, _ in inter]
    return dict(key=key, inter=inter, key_h=key_h, inter_h=inter_h, natural=key_h[0:3])


def test_histogram_restated_is_the_packers(pools, builtin, builtin_setup):
    """tests/enc_huff_ref.hist_of_words against the restatement's own table choice: the tables of least bits over the histogram are
    the ones enc_ref.encode_frame chose, and the histogram counts tokens_merged tokens."""
    for r, h in zip(pools["key"], pools["key_h"]):
        assert int(h.sum()) == r["tokens_merged"]
        for c in range(4):
            groups = range(1, 5) if c >> 1 else range(0, 1)
            cost = [sum(int(h[hg, c & 1] @ builtin[16 * hg + t, :, 1]) for hg in groups) for t in range(16)]
            assert int(np.argmin(cost)) == r["huff"][c]


# ---- headers -------------------------------------------------------------------------------------------------------------------------
def _bits(packet):
    return "".join(format(b, "08b") for b in packet)


def test_headers_state_the_codes(builtin, pools, tmp_path_factory, tmp_path):
    from oracle import ref
    E = _E()
    trained, _ = E.train_huffman(pools["key_h"] + pools["inter_h"])
    sets = dict(builtin=builtin, comb=HR.comb_codes(HR.comb_order), rotated=HR.rotated_codes(builtin), trained=trained)
    steps = hufftrain_host.Steps()
    plain = _enc().header_packets()
    for name, codes in sets.items():
        assert HR.valid(codes), name
        steps.valid(codes)
        steps.trees(codes)
        e = _enc(huffman=codes)
        hdr = e.header_packets()
        assert np.array_equal(e.huffman_codes(), codes), name
        e.close()
        sp = enc_ref.SetupParams(hdr[2])
        assert np.array_equal(HR.codes_of_setup(sp), codes), name
        trees = HR.tree_bits(codes)
        assert _bits(hdr[2])[sp.bits_used - len(trees):sp.bits_used] == trees, name
        assert len(hdr[2]) * 8 - sp.bits_used < 8
        # nothing else of the headers moves
        psp = enc_ref.SetupParams(plain[2])
        assert hdr[:2] == plain[:2] and sp.bits_used - len(trees) == psp.bits_used - len(HR.tree_bits(builtin))
        assert _bits(hdr[2])[:sp.bits_used - len(trees)] == _bits(plain[2])[:sp.bits_used - len(trees)], name
        if name == "builtin":
            assert hdr == plain
        if ref.available():
            rcs, info, setup, tc = ref.headerin(hdr)
            RL = ref.lib()
            RL.th_setup_free(setup)
            RL.th_comment_clear(C.byref(tc))
            assert all(rc > 0 for rc in rcs), (name, rcs)
            r = ref.RefEncoder(W, H, 0, quality=32)
            buf = E._huff_codes_in(codes)
            assert r._L.th_encode_ctl(r._enc, 0, C.byref(buf), C.sizeof(buf)) == 0
            rh = r.header_packets()
            r.close()
            rsp = enc_ref.SetupParams(rh[2])
            assert _bits(rh[2])[rsp.bits_used - len(trees):rsp.bits_used] == trees, name   # the tail, from the first tree on
            assert np.array_equal(HR.codes_of_setup(rsp), codes)
    got = steps.run(hufftrain_host.build(tmp_path_factory), tmp_path)
    for k, (name, codes) in enumerate(sets.items()):
        assert got[2 * k]["ok"] == 1
        assert got[2 * k + 1]["bits"] == HR.tree_bits(codes) and got[2 * k + 1]["nbits"] == len(HR.tree_bits(codes)), name


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
def _train_cases(pools, builtin):
    rng = np.random.default_rng(4)
    big = rng.integers((1 << 32) - 64, 1 << 32, (3, 5, 2, 32), dtype=np.int64)
    big[1, :, :, 7:] = rng.integers(0, 50, (5, 2, 25))
    one = pools["key_h"][1]
    comb = HR.comb_codes(HR.comb_order)
    return [("key", pools["key_h"], builtin, 8), ("natural", pools["natural"], builtin, 8), ("inter", pools["inter_h"], builtin, 8),
            ("mixed", pools["key_h"] + pools["inter_h"], builtin, 64), ("mixed from comb", pools["key_h"][::2] + pools["inter_h"][::3], comb, 3),
            ("none", [], HR.rotated_codes(builtin), 8), ("one", [one], builtin, 8), ("all equal", [one] * 7, builtin, 8),
            ("one round", pools["key_h"], builtin, 1), ("near 2^32", list(big), builtin, 8)]


def test_trainer_three_ways(pools, builtin, tmp_path_factory, tmp_path):
    E = _E()
    cases = _train_cases(pools, builtin)
    steps = hufftrain_host.Steps()
    for _, hists, start, rounds in cases:
        steps.train(hists, start, rounds)
    got = steps.run(hufftrain_host.build(tmp_path_factory), tmp_path)
    for (name, hists, start, rounds), host in zip(cases, got):
        want, wst = HR.train(hists, start, rounds)
        codes, st = E.train_huffman(hists, start, rounds)
        assert st == wst, name
        assert np.array_equal(codes, want), name
        assert host["rc"] == 0 and np.array_equal(host["codes"], want), name
        assert {k: host[k] for k in wst} == wst, name
        assert st["bits_end"] <= st["bits_start"], name
        assert HR.valid(codes) and codes[..., 1].max() <= 31, name
        if name == "none":
            assert np.array_equal(codes, start) and st["samples"] == 0
        if name == "natural":
            assert st["bits_end"] < st["bits_start"]
        if name == "key":   # start = None is the built-in codes
            c2, s2 = E.train_huffman(hists, None, rounds)
            assert np.array_equal(c2, codes) and s2 == st
    # refusals
    for hists, start, rounds in (([], None, 0), ([], None, 65), ([], _malformed(builtin)["nbits 33"], 8)):
        with pytest.raises(ValueError):
            E.train_huffman(hists, start, rounds)
    L = E._lib.load()
    out = E.HuffCodes()
    assert L.thip_huff_train(None, (1 << 20) + 1, None, 8, out, None) < 0
    assert L.thip_huff_train(None, 1, None, 8, out, None) == -1 and L.thip_huff_train(None, 0, None, 8, None, None) == -1


# ---- lossless ------------------------------------------------------------------------------------------------------------------------
def _code_bits(hist, codes):
    """The code bits of a packet with this histogram under the tables of least bits (what the packet writer chooses)."""
    total = 0
    for c in range(4):
        groups = range(1, 5) if c >> 1 else range(0, 1)
        total += min(sum(int(hist[hg, c & 1] @ codes[16 * hg + t, :, 1]) for hg in groups) for t in range(16))
    return total


def test_trained_codes_are_lossless(pools, builtin, builtin_setup):
    """The restatements' streams with trained codes: the same pictures in the reference decoder, plane for plane, and -- the
    training set being the clip itself -- bits_start - bits_end fewer token bits, exactly."""
    from oracle import ref
    E = _E()
    # key frames
    codes, st = E.train_huffman(pools["key_h"])
    setup = _setup_of(codes)
    trained = _run_key(setup)
    saved = 0
    for a, b, h in zip(pools["key"], trained, pools["key_h"]):
        assert np.array_equal(a["levels"], b["levels"]) and np.array_equal(a["words"], b["words"])
        saved += 8 * (len(a["packet"]) - len(b["packet"]))
        assert _code_bits(h, builtin) - _code_bits(h, codes) - 8 * (len(a["packet"]) - len(b["packet"])) in range(-7, 8)
    assert sum(_code_bits(h, builtin) - _code_bits(h, codes) for h in pools["key_h"]) == st["bits_start"] - st["bits_end"]
    assert st["bits_end"] < st["bits_start"] and saved > 0
    # inter frames: the reconstruction is the restatement's own decoder (the oracle); the packets go to the reference decoder too
    icodes, ist = E.train_huffman(pools["inter_h"])
    isetup = _setup_of(icodes)
    itrained = _run_inter(isetup)
    for (pa, ha, ra), (pb, hb, rb) in zip(pools["inter"], itrained):
        assert np.array_equal(ha, hb) and all(np.array_equal(x, y) for x, y in zip(ra, rb))
        assert (len(pa) == 0) == (len(pb) == 0)
    assert sum(_code_bits(h, builtin) - _code_bits(h, icodes) for h in pools["inter_h"]) == ist["bits_start"] - ist["bits_end"]
    if ref.available():
        for cs, key_pk, inter_pk in ((builtin, pools["key"], pools["inter"]), (None, trained, itrained)):
            kh = _enc(huffman=codes if cs is None else cs).header_packets()
            pics = []
            for r in key_pk:
                rd = ref.RefDecoder(kh)
                assert rd.packetin(r["packet"])[0] == 0
                pics.append(rd.ycbcr_out())
                rd.close()
            ih = _enc(huffman=icodes if cs is None else cs).header_packets()
            for k in range(0, len(inter_pk), 6):
                rd = ref.RefDecoder(ih)
                for pkt, _, recon in inter_pk[k:k + 6]:
                    assert rd.packetin(pkt)[0] >= 0
                    pic = rd.ycbcr_out()
                    assert not refcmp.diff_planes(pic, recon)
                    pics.append(pic)
                rd.close()
            if cs is None:
                assert len(pics) == len(first) and all(not refcmp.diff_planes(a, b) for a, b in zip(first, pics))
            first = pics
