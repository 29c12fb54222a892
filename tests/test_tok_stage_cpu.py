"""tests/tok_stage_ref.py, the restatement of thip_enc_tok_stage, pinned to the packets of enc_ref and enc_inter_ref; the entry's
refusals; and the proof that the inputs tests/test_gpu_tok_direct.py feeds the kernels take every branch they are meant to."""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

from tests import enc_inter_ref, enc_ref
from tests import tok_stage_ref as T
from theora_amd import _lib
from theora_amd.encoder import Encoder, tok_stage

_setup = None


def _setup_params():
    global _setup
    if _setup is None:
        e = Encoder(64, 48, 0, 32)
        _setup = enc_ref.SetupParams(e.header_packets()[2])
        e.close()
    return _setup


def _raster_dc(geo, levels):
    dcq = np.zeros(geo.nfrags, np.int64)
    dcq[geo.coded_order] = np.asarray(levels)[:, 0]
    return dcq


# ---- the restatement is the packets' -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,w,h,fmt,qi", [("flat", 48, 32, 0, 20), ("noise", 48, 32, 0, 40), ("natural", 64, 48, 0, 30),
                                               ("noise", 32, 32, 3, 63), ("natural", 48, 32, 2, 10), ("noise", 16, 16, 0, 50)])
def test_key_restatement_is_enc_refs(kind, w, h, fmt, qi):
    """On enc_ref.encode_frame's own levels the three stages give that frame's words and list lengths, and the sorted order is the
    scattered one."""
    if kind == "natural":
        frame = enc_ref.picture(kind, w, h, fmt, (0, 0, w, h), seed=w + qi)
    else:
        frame = [np.full(s, 128, np.uint8) if kind == "flat" else enc_ref.content("noise", s, 5) for s in enc_ref.plane_shapes(w, h, fmt)]
    ref = enc_ref.encode_frame(frame, w, h, fmt, (0, 0, w, h), qi, _setup_params())
    geo = T.geometry(w, h, fmt)
    assert np.array_equal(geo.coded_order, ref["coded_order"])
    r = T.restate(geo, 0, ref["levels"], dcq=_raster_dc(geo, ref["levels"]))
    assert np.array_equal(r["out"], ref["words"])
    assert np.array_equal(r["list_len"].astype(np.int64), ref["list_len"].T)
    assert np.array_equal(T.stream_words(r), ref["words"])
    assert r["overflow"] == 0 and int(r["ntok"].sum()) == ref["tokens"]
    assert np.array_equal(r["chunk_cnt"].astype(np.int64).sum(0), ref["list_len"].T)


@pytest.mark.parametrize("kind,w,h,fmt,qi", [("pan", 64, 48, 0, 30), ("static", 48, 32, 0, 40), ("cut", 64, 48, 3, 20)])
def test_inter_restatement_is_enc_inter_refs(kind, w, h, fmt, qi):
    frames = enc_inter_ref.sequence(kind, w, h, fmt, 4, seed=3)
    enc = enc_inter_ref.InterEncoder(w, h, fmt, (0, 0, w, h), _setup_params(), 64, 6)
    geo = T.geometry(w, h, fmt)
    seen = 0
    for fr in frames:
        ref = enc.frame(fr, qi)
        if ref["key"] or not ref["packet"]:
            continue
        rng = np.random.default_rng(seen)
        levels = ref["levels"].copy()
        unc = ref["cmap"][geo.coded_order] == 0
        levels[unc] = rng.integers(-600, 601, (int(unc.sum()), 64))   # (an uncoded block's levels are not read)
        r = T.restate(geo, 2, levels, dcr=ref["dcr"], cmap=ref["cmap"])
        assert np.array_equal(r["out"], ref["words"])
        assert np.array_equal(r["list_len"].astype(np.int64), ref["list_len"].T)
        assert np.array_equal(T.stream_words(r), ref["words"])
        assert int(r["ntok"].sum()) == ref["tokens"] and not r["ntok"][unc].any() and not r["mask"][unc].any()
        seen += 1
    enc.close()
    assert seen >= 2


def test_own_dc_is_the_levels_and_the_neighbours_are_dcqs():
    geo = T.geometry(64, 48, 0)
    rng = np.random.default_rng(1)
    dcq = T.dc_frame(geo, 1)
    lv = np.zeros((geo.nfrags, 64), np.int16)
    lv[:, 0] = rng.integers(-300, 301, geo.nfrags)
    res = T.key_residuals(geo, lv, dcq)
    same = lv.copy()
    same[:, 0] = dcq[geo.coded_order]
    assert np.array_equal(res - T.key_residuals(geo, same, dcq), lv[:, 0].astype(np.int64) - dcq[geo.coded_order])


def test_banded_dc_prediction_is_the_whole_planes():
    rng = np.random.default_rng(2)
    for nh, nv in ((5, 40), (1, 9), (7, 1)):
        q = np.zeros((nv, nh), np.int64)
        for fy in rng.integers(0, nv, 4):
            q[fy] = rng.integers(-500, 501, nh)
        q[nv - 1, nh - 1] = 77
        assert np.array_equal(T._plane_residuals(q.reshape(-1), nh, nv), enc_ref.dc_predict(q.reshape(-1), nh, nv))


def test_scan_and_scatter_on_a_hand_made_frame():
    """Two chunks; index 5 has tokens in blocks 3 and 255 of chunk 0 and block 256, index 0 in block 256 alone."""
    n = 300
    tok = np.zeros((n, 65), np.uint32)
    mask = np.zeros(n, np.uint64)
    cnt = np.zeros((2, 3, 64), np.uint32)
    for k, zs in ((3, (5,)), (255, (5,)), (256, (0, 5))):
        for i, z in enumerate(zs):
            tok[k, i] = 1000 * k + z
            mask[k] |= np.uint64(1 << z)
            cnt[k // 256, 1, z] += 1
    base, ll = T.scan(cnt)
    assert base[1, 5] == 2 and base[1, 0] == 0 and ll[1, 5] == 3 and ll[1, 0] == 1 and int(ll.sum()) == 4
    out, written, clash = T.scatter(tok, mask, base, ll)
    assert list(out) == [256000, 3005, 255005, 256005] and written.all() and not clash


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
_A = 0x10000   # a device address that is never followed: every refusal here comes before a device is touched

_ALL = dict(levels=_A, dcq=_A, dcr=_A, cmap=_A, tok=_A, mask=_A, chunk_cnt=_A, chunk_base=_A, list_len=_A, overflow=_A, out=_A, out_cap=1 << 20)


def _call(frame=(64, 48), fmt=0, classes=0, stages=7, **kw):
    return tok_stage(frame, fmt, classes, stages, **{**_ALL, **kw})


def test_refusals():
    L = _lib.load()
    assert L.thip_enc_tok_stage(None) == _lib.EFAULT
    for st in (0, 8, -1, 15):
        assert _call(stages=st) == _lib.EINVAL, st
    for frame in ((0, 48), (64, 0), (-16, 48), (60, 48), (64, 40), (1 << 20, 16), (16, 1 << 20)):
        assert _call(frame=frame) == _lib.EINVAL, frame
    assert _call(frame=(1 << 15, 1 << 15), fmt=3) == _lib.EINVAL        # 3 * 2^24 fragments
    assert _call(frame=(1 << 15, 1 << 15), fmt=0) == _lib.EINVAL        # 1.5 * 2^24
    for fmt in (-1, 1, 4):
        assert _call(fmt=fmt) == _lib.EINVAL, fmt
    for classes in (-1, 1, 4):
        assert _call(classes=classes) == _lib.EINVAL, classes
    # a NULL for anything a requested stage reads or writes; what no requested stage touches may be NULL
    needs = {1: {0: ("levels", "dcq", "tok", "mask", "chunk_cnt", "overflow"), 2: ("levels", "dcr", "cmap", "tok", "mask", "chunk_cnt", "overflow")},
             2: {0: ("chunk_cnt", "chunk_base", "list_len")}, 4: {0: ("tok", "mask", "chunk_base", "list_len", "out")}}
    for st, by_class in needs.items():
        for classes, need in by_class.items():
            for name in need:
                assert _call(stages=st, classes=classes, **{name: None}) == _lib.EFAULT, (st, classes, name)
                assert _call(stages=7, classes=classes, **{name: None}) == _lib.EFAULT, (7, classes, name)
    for name, a in (("levels", 2), ("levels", 8), ("dcq", 1), ("dcr", 1), ("tok", 2), ("mask", 4), ("chunk_cnt", 2), ("chunk_base", 1),
                    ("list_len", 2), ("overflow", 2), ("out", 2)):
        assert _call(classes=2 if name == "dcr" else 0, **{name: _A + a}) == _lib.EINVAL, (name, a)
    assert _call(cmap=_A + 1, classes=2, levels=_A + 4) == _lib.EINVAL   # (cmap has no alignment; levels is what is refused)


def test_struct_matches_the_header(tmp_path):
    """sizeof and offsetof of thip_enc_tok_req as a C compiler lays the header's struct out == the ctypes structure."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in _lib.EncTokReq._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "theora_hip.h"\nint main(void) {\n  printf("%zu", sizeof(thip_enc_tok_req));\n' +
                   "".join('  printf(" %%zu", offsetof(thip_enc_tok_req, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.EncTokReq)] + [getattr(_lib.EncTokReq, f).offset for f in fields]


# ---- the GPU tests' inputs take the branches they claim ----------------------------------------------------------------------------
def _key_cover(geo, levels, dcq):
    return T.tokens(geo, 0, levels, dcq=dcq)["cover"]


def test_rule_cases_reach_every_token_branch_and_value_class():
    from tests.test_gpu_tok_direct import rule_frames
    geo = T.geometry(64, 48, 0)
    cover = set()
    for levels, dcq in rule_frames():
        cover |= _key_cover(geo, levels, dcq)
    toks = {c[1] for c in cover if c[0] == "tok"}
    assert toks == {0, "no-eob"} | set(range(7, 32)), sorted(map(str, toks))
    gaps = {c[1:] for c in cover if c[0] == "gap"}
    assert set(T.RULE_EDGES) <= gaps, sorted(set(T.RULE_EDGES) - gaps)
    values = {c[1] for c in cover if c[0] == "value"}
    assert {s * v for v in T.VALUES for s in (1, -1)} <= values
    # a combined token's run at the block's first and last index that holds it
    assert (1, 63) in gaps and (4, 63) in gaps


def test_dc_frames_reach_every_predictor_branch():
    from tests.test_gpu_tok_direct import DC_FRAMES, dc_case
    per_frame = {}
    for w, h, fmt in DC_FRAMES:
        geo = T.geometry(w, h, fmt)
        cover = set()
        for seed in range(3):
            levels, dcq = dc_case(geo, seed)
            cover |= _key_cover(geo, levels, dcq)
        per_frame[(w, h, fmt)] = cover
    small = set().union(*(per_frame[(16, 16, f)] for f in (0, 2, 3)))
    assert {c[1] for c in small if c[0] == "mask"} == {0, 1, 4, 7, 12}          # (16x16: no plane is three fragments wide)
    assert ("mask", 4) in per_frame[(16, 16, 2)]                                  # (a plane one fragment wide and two high)
    for key in ((64, 48, 0), (48, 80, 0)):
        cover = per_frame[key]
        assert {c[1] for c in cover if c[0] == "mask"} == {0, 1, 7, 12, 15}, key
        assert {c[1] for c in cover if c[0] == "fallback"} == {"none", "u", "l", "ul", "u before l", "l before ul"}, (key, cover)
        assert {c[1] for c in cover if c[0] == "div32"} == {1, -1}, key
    # a chroma plane one fragment wide and high (4:2:0), one wide and two high (4:2:2)
    assert [(g["nhfrags"], g["nvfrags"]) for g in T.geometry(16, 16, 0).planes] == [(2, 2), (1, 1), (1, 1)]
    assert [(g["nhfrags"], g["nvfrags"]) for g in T.geometry(16, 16, 2).planes] == [(2, 2), (1, 2), (1, 2)]


def test_dc_cases_hold_both_kinds_of_disagreement():
    """A DC level of zero with a non-zero residual, a non-zero DC level with a zero residual, and levels[k][0] unlike dcq."""
    from tests.test_gpu_tok_direct import dc_case
    geo = T.geometry(64, 48, 0)
    seen = set()
    for seed in range(3):
        levels, dcq = dc_case(geo, seed)
        res = T.key_residuals(geo, levels, dcq)
        own = levels[:, 0].astype(np.int64)
        seen |= {"zero level, residual" for _ in [0] if ((own == 0) & (res != 0)).any()}
        seen |= {"level, zero residual" for _ in [0] if ((own != 0) & (res == 0)).any()}
        seen |= {"levels unlike dcq" for _ in [0] if (own != dcq[geo.coded_order]).any()}
    assert len(seen) == 3, seen


def test_overflow_cases_overflow():
    from tests.test_gpu_tok_direct import overflow_case
    geo = T.geometry(64, 48, 0)
    levels, dcq = overflow_case(geo)
    t = T.tokens(geo, 0, levels, dcq=dcq)
    assert ("tok", "overflow") in t["cover"] and {("value", 581), ("value", -581)} <= t["cover"]
    big = np.abs(levels.astype(np.int64)) > 580
    assert t["overflow"] == int(big[:, 1:].sum()) + int((np.abs(t["values"][:, 0]) > 580).sum()) >= 8
    assert (big.sum(1) > 1).any() and len({int(p) for p in t["plane"][big.any(1)]}) == 3
    words = t["tok"][np.arange(65)[None, :] < t["ntok"][:, None]]
    assert ((words & 31 == 22) & ((words >> 5) & 0x1FF == 511)).sum() >= t["overflow"]


def test_large_frames_are_the_sizes_they_claim():
    from tests.test_gpu_tok_direct import LARGE
    sizes = {(w, h): T.geometry(w, h, 0).nfrags for (w, h) in LARGE}
    assert sizes[(1408, 1984)] == 65472 == 256 * 256 - 64 and T.nchunks(65472) == 256
    assert sizes[(1536, 1824)] == 65664 and T.nchunks(65664) == 257
    # the last chunk with a single live block: n = 1.5 (w / 8)(h / 8) = 6 mbs with mbs = (w / 16)(h / 16), so n mod 256 is even
    # whatever the size in 4:2:0 -- 1 does not exist; the least remainder there is 2
    assert all((6 * m) % 256 != 1 for m in range(1, 20000))
    assert sizes[(16, 688)] == 258 and 258 % 256 == 2
    # 4:4:4 gives n = 12 mbs, 4:2:2 n = 8 mbs: even too
    t0 = time.time()
    geo = T.geometry(1536, 1824, 0)
    rng = np.random.default_rng(0)
    lv = T.sparse_levels(geo.nfrags, T.seam_blocks(geo.nfrags, (0, 1, 255, 256), rng), rng)
    r = T.restate(geo, 0, lv, dcq=_raster_dc(geo, lv), want_cover=False)
    assert len(r["out"]) == int(r["ntok"].sum()) >= geo.nfrags
    assert time.time() - t0 < 20   # (usable at this size: about a second)
