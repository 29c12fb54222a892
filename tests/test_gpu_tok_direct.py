"""The tokeniser of th_encode_* (k_enc_intra_tok, k_enc_inter_tok, k_enc_intra_scan, k_enc_intra_scatter of
theora_amd/csrc/thip_encode.h and thip_encode_inter.h) driven directly, through thip_enc_tok_stage, at every token, DC and chunk
edge: synthetic levels, DCs, maps, counts and masks fix what a picture would otherwise have to land on.  Every comparison is exact
equality with tests/tok_stage_ref.py.  Every output buffer is longer than the entry may use and filled with a pattern; the words
behind a block's tokens, behind the stream's last token and behind each array's end must still hold it.

tests/test_tok_stage_cpu.py proves that the generators here reach the branches they are meant to."""
import numpy as np
import pytest

from tests import tok_stage_ref as T

pytestmark = pytest.mark.gpu

PAT, PAD = 0x5A5A5A5A, 67
TOK, SCAN, SCATTER = 1, 2, 4
WORDS = {"tok": lambda n, c: n * 65, "mask": lambda n, c: 2 * n, "chunk_cnt": lambda n, c: c * 192, "chunk_base": lambda n, c: c * 64,
         "list_len": lambda n, c: 192, "overflow": lambda n, c: 1}
WRITES = {TOK: ("tok", "mask", "chunk_cnt", "overflow"), SCAN: ("chunk_base", "list_len"), SCATTER: ("out",)}
INT = {"levels": np.int16, "dcq": np.int16, "dcr": np.int16, "cmap": np.uint8}


def run(frame, fmt, classes, stages, out_cap=0, given=None, **inputs):
    """One call of the entry.  inputs: levels, dcq, dcr, cmap (numpy); given: the buffers a stage that does not run would have left
    (numpy, by the entry's names).  What a requested stage writes is allocated, PAD words longer than it may use, and filled with
    PAT.  Returns (return code, {name: uint32 words as they came back, the padding checked and cut off})."""
    import torch
    from theora_amd.encoder import tok_stage
    geo = T.geometry(frame[0], frame[1], fmt)
    n, c = geo.nfrags, T.nchunks(geo.nfrags)
    size = {k: f(n, c) for k, f in WORDS.items()}
    size["out"] = out_cap
    dev = {}
    for k, a in inputs.items():
        dev[k] = torch.from_numpy(np.ascontiguousarray(a, INT[k]).reshape(-1).view(np.int8 if k == "cmap" else np.int16)).cuda()
    wanted = [k for s, ks in WRITES.items() if stages & s for k in ks] + list(given or {})
    for k in dict.fromkeys(wanted):
        dev[k] = torch.full((size[k] + PAD,), PAT, dtype=torch.int32, device="cuda")
        if given and k in given:
            a = np.ascontiguousarray(given[k]).reshape(-1)
            a = a.view(np.uint32) if a.dtype == np.uint64 else a.astype(np.uint32)
            assert a.size == size[k], (k, a.size, size[k])
            dev[k][:size[k]] = torch.from_numpy(a.view(np.int32)).cuda()
    torch.cuda.synchronize()
    rc = tok_stage(frame, fmt, classes, stages, out_cap=out_cap, **{k: t.data_ptr() for k, t in dev.items()})
    got = {}
    for k in size:
        if k in dev:
            a = dev[k].cpu().numpy().view(np.uint32)
            assert (a[size[k]:] == PAT).all(), "%s: written behind its end" % k
            got[k] = a[:size[k]]
    return rc, got


def same(name, got, want):
    got = np.asarray(got).reshape(-1)
    want = np.broadcast_to(want, got.shape) if np.ndim(want) == 0 else np.asarray(want).reshape(-1)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s: %d of %d differ, first at %d: %#x for %#x" % (name, len(bad), len(got), bad[0], int(got[bad[0]]), int(want[bad[0]])))


def check_tok(got, r):
    """Stage TOK's outputs against tokens()'s: a block's words as far as it has tokens, the pattern behind them."""
    n = len(r["ntok"])
    want = np.full((n, 65), PAT, np.uint32)
    live = np.arange(65)[None, :] < r["ntok"][:, None]
    want[live] = r["tok"][live]
    same("tok", got["tok"], want)
    coded = np.repeat(r["coded"], 2)
    same("mask", got["mask"][coded], r["mask"].view(np.uint32)[coded])
    same("mask of uncoded blocks", got["mask"][~coded], 0)
    same("chunk_cnt", got["chunk_cnt"], r["chunk_cnt"])
    same("overflow", got["overflow"], r["overflow"])


def check_all(frame, fmt, classes, slack=9, **inputs):
    """All three stages in one call against restate(); returns (the restatement, what came back)."""
    geo = T.geometry(frame[0], frame[1], fmt)
    r = T.restate(geo, classes, inputs["levels"], inputs.get("dcq"), inputs.get("dcr"), inputs.get("cmap"), want_cover=False)
    total = len(r["out"])
    rc, got = run(frame, fmt, classes, TOK | SCAN | SCATTER, out_cap=total + slack, **inputs)
    assert rc == 0
    check_tok(got, r)
    same("chunk_base", got["chunk_base"], r["chunk_base"])
    same("list_len", got["list_len"], r["list_len"])
    same("out", got["out"][:total], r["out"])
    same("out behind the last token", got["out"][total:], PAT)
    return r, got


def raster(geo, per_block):
    a = np.zeros(geo.nfrags, np.asarray(per_block).dtype)
    a[geo.coded_order] = per_block
    return a


# ---- the token rule ----------------------------------------------------------------------------------------------------------------
RULE = (64, 48, 0)   # 72 blocks a frame


def rule_frames():
    """(levels, dcq) of every 64x48 frame of the token-rule cases; dcq is zero, so a block's DC residual is its levels[k][0]."""
    rng = np.random.default_rng(11)
    blocks = np.concatenate([T.rule_blocks(T.rule_cases(12, 500)), T.shaped_blocks(rng)])
    n = T.geometry(*RULE).nfrags
    blocks = np.concatenate([blocks, np.zeros((-len(blocks) % n, 64), np.int16)])
    return [(blocks[i:i + n], np.zeros(n, np.int16)) for i in range(0, len(blocks), n)]


@pytest.mark.parametrize("part", range(4))
def test_token_rule_and_its_copy(hip, part):
    """Every boundary of the rule at the block's first, a middle and its last index that holds it, in k_enc_intra_tok; the same
    levels through k_enc_inter_tok (every block coded, dcr the key frame's residual) give the same words: the rule's two copies."""
    geo = T.geometry(*RULE)
    frames = rule_frames()
    for levels, dcq in frames[part::4]:
        r, key = check_all(RULE[:2], RULE[2], 0, levels=levels, dcq=dcq)
        dcr = raster(geo, r["values"][:, 0].astype(np.int16))
        _, inter = check_all(RULE[:2], RULE[2], 2, levels=levels, dcr=dcr, cmap=np.full(geo.nfrags, 2, np.uint8))
        for k in key:
            same("key and inter " + k, key[k], inter[k])


# ---- DC prediction -------------------------------------------------------------------------------------------------------------------
DC_FRAMES = [(16, 16, 0), (16, 16, 2), (16, 16, 3), (64, 48, 0), (48, 80, 0)]


def dc_case(geo, seed):
    """(levels, dcq): dcq takes the predictor's branches (tok_stage_ref.dc_frame), with a constant patch where the plane has room
    (a DC predicted exactly: a level with no residual) and zeros among its neighbours (no level, a residual); one block in three
    carries a DC in levels unlike its dcq; a few AC levels everywhere.  A plane of at least 6 x 5 fragments also holds the three
    fallbacks of the weighted predictor by hand."""
    rng = np.random.default_rng(100 + seed)
    dcq = T.dc_frame(geo, seed).copy()
    for g in geo.planes:
        q = dcq[g["froffset"]:g["froffset"] + g["nfrags"]].reshape(g["nvfrags"], g["nhfrags"])
        if min(q.shape) >= 3:
            q[:3, :3] = 37
            q[-1, -2] = 0
        if q.shape[0] >= 5 and q.shape[1] >= 6:   # (ul, u over l, the block): the fallback to ul; u where l fails too; l where ul fails too
            q[3:5, 0:2] = [[250, 400], [400, 9]]
            q[3:5, 2:4] = [[-400, 402], [400, -9]]
            q[3:5, 4:6] = [[-390, 300], [-400, 0]]
    levels = T.sparse_levels(geo.nfrags, range(0, geo.nfrags, 2), rng)
    levels[:, 0] = dcq[geo.coded_order]
    odd = rng.random(geo.nfrags) < 1 / 3
    odd[geo.coded_order.tolist().index(geo.planes[0]["froffset"] + geo.planes[0]["nhfrags"] + 1)] = False   # (the patch's middle)
    levels[odd, 0] = rng.integers(-300, 301, int(odd.sum()))
    return levels, dcq


@pytest.mark.parametrize("w,h,fmt", DC_FRAMES)
def test_dc_prediction(hip, w, h, fmt):
    geo = T.geometry(w, h, fmt)
    for seed in range(3):
        levels, dcq = dc_case(geo, seed)
        check_all((w, h), fmt, 0, levels=levels, dcq=dcq)


# ---- overflow ------------------------------------------------------------------------------------------------------------------------
def overflow_case(geo):
    """Levels beyond +-580 in the first and last block of every plane and on both sides of every chunk edge: +-581, +-32767,
    -32768, up to five in a block, and a DC whose residual alone is beyond (dcq is zero)."""
    n = geo.nfrags
    levels = np.zeros((n, 64), np.int16)
    vals = (581, -581, 32767, -32767, -32768)
    first = np.concatenate([[0], np.nonzero(np.diff(geo.plane_of[geo.coded_order]))[0] + 1])
    ks = sorted(set(first.tolist()) | set((first[1:] - 1).tolist()) | {n - 1} | {k for e in range(256, n, 256) for k in (e - 1, e)})
    for i, k in enumerate(ks):
        m = 1 + i % 5
        levels[k, [1 + 7 * j + i % 6 for j in range(m)]] = [vals[(i + j) % 5] for j in range(m)]
        levels[k, 40] = 580 if i & 1 else -580
    levels[ks[0], 0] = 600
    levels[ks[-1], 0] = -32768
    return levels, np.zeros(n, np.int16)


@pytest.mark.parametrize("w,h", [(64, 48), (80, 272)])
def test_overflow_is_counted_and_clamped(hip, w, h):
    geo = T.geometry(w, h, 0)
    levels, dcq = overflow_case(geo)
    r, got = check_all((w, h), 0, 0, levels=levels, dcq=dcq)
    assert int(got["overflow"][0]) == r["overflow"] >= 8
    words = got["out"][:len(r["out"])]
    clamped = (words & 31 == 22) & ((words >> 5) & 0x1FF == 511)
    assert int(clamped.sum()) == r["overflow"] + int((np.abs(r["values"]) == 580).sum())
    # the same through the inter kernel, the DC's overflow in dcr
    dcr = raster(geo, np.clip(r["values"][:, 0], -32768, 32767).astype(np.int16))
    r2, got2 = check_all((w, h), 0, 3, levels=levels, dcr=dcr, cmap=np.full(geo.nfrags, 3, np.uint8))
    assert int(got2["overflow"][0]) == r2["overflow"] == r["overflow"]


# ---- chunks and the scan -------------------------------------------------------------------------------------------------------------
# frame: the chunks whose seams get levels.  1408x1984 is 65472 blocks, exactly 256 chunks (one pass of the scan, all lanes live);
# 1536x1824 is 65664, 257 chunks (the scan's second pass, with one live lane); 16x688 is 258 blocks and 80x272 is 510: the last
# chunk with 2 and with 254 live blocks -- n = 1.5 (w / 8)(h / 8) is even for every frame, so 1 and 255 do not exist
LARGE = {(1408, 1984): (0, 1, 127, 254, 255), (1536, 1824): (0, 1, 255, 256), (16, 688): (0, 1), (80, 272): (0, 1)}


def large_case(w, h):
    geo = T.geometry(w, h, 0)
    rng = np.random.default_rng(w + h)
    levels = T.sparse_levels(geo.nfrags, T.seam_blocks(geo.nfrags, LARGE[(w, h)], rng, 150), rng)
    dcq = raster(geo, levels[:, 0].copy())
    return geo, levels, dcq


@pytest.mark.parametrize("w,h", sorted(LARGE))
def test_chunk_seams_in_a_key_frame(hip, w, h):
    geo, levels, dcq = large_case(w, h)
    r, _ = check_all((w, h), 0, 0, levels=levels, dcq=dcq)
    assert int(r["list_len"].sum()) >= geo.nfrags


def test_plane_boundaries_inside_one_chunk(hip):
    """64x48: luma's 48 blocks and both chroma planes' 12 share chunk 0 and its counters."""
    geo = T.geometry(64, 48, 0)
    rng = np.random.default_rng(5)
    levels = rng.integers(-5, 6, (geo.nfrags, 64)).astype(np.int16) * (rng.random((geo.nfrags, 64)) < 0.4)
    r, _ = check_all((64, 48), 0, 0, levels=levels.astype(np.int16), dcq=T.dc_frame(geo, 0))
    assert (r["chunk_cnt"][0].sum(1) > 0).all()


SCAN_FRAMES = {1: (64, 48), 255: (2048, 1360), 256: (1408, 1984), 257: (1536, 1824), 512: (1792, 3120), 513: (2048, 2736)}


@pytest.mark.parametrize("chunks", sorted(SCAN_FRAMES))
def test_scan_alone_on_made_up_counts(hip, chunks):
    """k_enc_intra_scan on counts no picture produces: up to 2^20 a cell, zeros, one index empty throughout, one (plane, index)
    empty; 1, 255, 256 chunks in one pass, 257, 512 in two, 513 in three."""
    w, h = SCAN_FRAMES[chunks]
    assert T.nchunks(T.geometry(w, h, 0).nfrags) == chunks
    rng = np.random.default_rng(chunks)
    cnt = rng.integers(0, (1 << 20) + 1, (chunks, 3, 64)).astype(np.uint32)
    cnt[rng.random(cnt.shape) < 0.3] = 0
    cnt[:, :, 17] = 0
    cnt[:, 1, 40] = 0
    cnt[chunks - 1, 2, 63] = 1 << 20
    rc, got = run((w, h), 0, 0, SCAN, given=dict(chunk_cnt=cnt))
    assert rc == 0
    base, ll = T.scan(cnt)
    same("chunk_base", got["chunk_base"], base)
    same("list_len", got["list_len"], ll)
    same("chunk_cnt is read only", got["chunk_cnt"], cnt)


def _made_up_scatter(w, h, masks):
    """tok, mask, chunk_base, list_len for the masks {block: indices}: every word names its block and place."""
    geo = T.geometry(w, h, 0)
    n = geo.nfrags
    tok = np.full((n, 65), 0xDEAD0000, np.uint32)
    mask = np.zeros(n, np.uint64)
    cnt = np.zeros((T.nchunks(n), 3, 64), np.int64)
    plane = geo.plane_of[geo.coded_order]
    for k, zs in masks.items():
        for i, z in enumerate(sorted(zs)):
            tok[k, i] = (k << 8 | z) & 0xFFFFFFFF
            mask[k] |= np.uint64(1 << z)
            cnt[k // 256, plane[k], z] += 1
    base, ll = T.scan(cnt)
    return dict(tok=tok, mask=mask, chunk_base=base, list_len=ll)


SCATTER_CASES = {
    "lanes 63 and 64": (80, 272, lambda n: {63: (0, 9), 64: (0, 9), 256 + 63: (9,), 256 + 64: (9, 63)}),
    "lanes 127 128 191 192": (80, 272, lambda n: {k: (3, 60) for k in (127, 128, 191, 192, 256 + 127, 256 + 128, 256 + 191, 256 + 192)}),
    "last live lane": (80, 272, lambda n: {n - 1: (0, 1, 63)}),
    "last live lane and the first": (16, 688, lambda n: {0: (5,), n - 1: (5,), n - 2: (5, 6)}),
    "index 0 in every block": (80, 272, lambda n: {k: (0,) for k in range(n)}),
    "every index in one wave's blocks": (64, 48, lambda n: {k: tuple(range(64)) for k in range(n)}),
    "nothing": (64, 48, lambda n: {}),
}


@pytest.mark.parametrize("name", sorted(SCATTER_CASES))
def test_scatter_alone_on_made_up_masks(hip, name):
    w, h, make = SCATTER_CASES[name]
    given = _made_up_scatter(w, h, make(T.geometry(w, h, 0).nfrags))
    want, written, clash = T.scatter(given["tok"], given["mask"], given["chunk_base"], given["list_len"])
    assert written.all() and not clash
    rc, got = run((w, h), 0, 0, SCATTER, out_cap=len(want) + 5, given=given)
    assert rc == 0
    same("out", got["out"][:len(want)], want)
    same("out behind the last token", got["out"][len(want):], PAT)
    for k in given:
        same(k + " is read only", got[k], np.ascontiguousarray(given[k]).reshape(-1).view(np.uint32) if k == "mask" else given[k])


def test_scatter_refuses_what_does_not_fit(hip):
    """The sum of list_len above out_cap, and a chunk_base that puts a token behind it: THIP_EINVAL, and out is not touched."""
    from theora_amd import _lib
    n = T.geometry(80, 272, 0).nfrags
    given = _made_up_scatter(80, 272, {k: (0, 7) for k in range(0, n, 3)})
    total = int(given["list_len"].sum())
    rc, got = run((80, 272), 0, 0, SCATTER, out_cap=total - 1, given=given)
    assert rc == _lib.EINVAL
    same("out", got["out"], PAT)
    rc, got = run((80, 272), 0, 0, SCATTER, out_cap=total, given=given)
    assert rc == 0 and not (got["out"] == PAT).any()
    bad = dict(given, chunk_base=given["chunk_base"].copy())
    bad["chunk_base"][1, 7] += 1
    rc, got = run((80, 272), 0, 0, SCATTER, out_cap=total, given=bad)
    assert rc == _lib.EINVAL
    same("out", got["out"], PAT)


def test_stages_read_the_callers_buffers(hip):
    """TOK then SCATTER in one call with SCAN left out: the scatter goes by the chunk_base and list_len given, not by the counts TOK
    has just made.  Nothing a stage does not touch is needed: the other pointers are NULL."""
    geo, levels, dcq = large_case(16, 688)
    r = T.restate(geo, 0, levels, dcq, want_cover=False)
    rc, got = run((16, 688), 0, 0, TOK, levels=levels, dcq=dcq)
    assert rc == 0 and set(got) == {"tok", "mask", "chunk_cnt", "overflow"}
    check_tok(got, r)
    rc, got = run((16, 688), 0, 0, TOK | SCATTER, out_cap=len(r["out"]), levels=levels, dcq=dcq,
                  given=dict(chunk_base=r["chunk_base"], list_len=r["list_len"]))
    assert rc == 0
    same("out", got["out"], r["out"])
    same("chunk_base", got["chunk_base"], r["chunk_base"])


# ---- inter frames ----------------------------------------------------------------------------------------------------------------------
INTER = (176, 144, 0)   # 594 blocks: chunks 0 and 1 whole, 82 blocks in chunk 2


def inter_case(classes, shape, seed):
    """(levels, dcr, cmap).  An uncoded block carries levels and a dcr beyond +-580 that must be neither tokens nor overflows."""
    geo = T.geometry(*INTER)
    n = geo.nfrags
    rng = np.random.default_rng(seed)
    cmap_k = rng.integers(0, classes + 1, n).astype(np.uint8)   # (coded order)
    if shape == "chunk 1 uncoded":
        cmap_k[256:512] = 0
    elif shape == "none coded":
        cmap_k[:] = 0
    elif shape == "one coded":
        cmap_k[:] = 0
        cmap_k[511] = classes
    levels = (rng.integers(-40, 41, (n, 64)) * (rng.random((n, 64)) < 0.15)).astype(np.int16)
    dcr_k = rng.integers(-300, 301, n).astype(np.int16)
    dcr_k[rng.random(n) < 0.3] = 0
    unc = cmap_k == 0
    levels[unc] = rng.integers(-32768, 32768, (int(unc.sum()), 64))
    dcr_k[unc] = 30000
    return geo, levels, raster(geo, dcr_k), raster(geo, cmap_k)


@pytest.mark.parametrize("classes", [2, 3])
@pytest.mark.parametrize("shape", ["random", "chunk 1 uncoded", "none coded", "one coded"])
def test_inter_frames(hip, classes, shape):
    geo, levels, dcr, cmap = inter_case(classes, shape, 7 * classes + len(shape))
    r, got = check_all(INTER[:2], INTER[2], classes, levels=levels, dcr=dcr, cmap=cmap)
    assert r["overflow"] == 0
    if shape == "none coded":
        assert not got["list_len"].any() and not got["chunk_cnt"].any() and (got["out"] == PAT).all() and (got["tok"] == PAT).all()
    if shape == "chunk 1 uncoded":
        assert not got["chunk_cnt"][192:384].any() and got["chunk_cnt"][:192].any() and got["chunk_cnt"][384:].any()


# ---- the stream's order, and the hand-over to the packetiser -------------------------------------------------------------------------
def test_stream_order_by_sorting(hip):
    """A dense frame: out is ordered by index, then plane, then coded order -- against the restatement, and against the blocks' own
    tokens as they came back, sorted as Python tuples."""
    geo = T.geometry(*INTER)
    rng = np.random.default_rng(21)
    levels = (rng.integers(-9, 10, (geo.nfrags, 64)) * (rng.random((geo.nfrags, 64)) < 0.5)).astype(np.int16)
    r, got = check_all(INTER[:2], INTER[2], 0, levels=levels, dcq=T.dc_frame(geo, 2))
    tok = got["tok"].reshape(-1, 65)
    plane = geo.plane_of[geo.coded_order]
    tuples = sorted(((int(tok[k, i]) >> 16) & 63, int(plane[k]), k, i) for k in range(geo.nfrags) for i in range(int(r["ntok"][k])))
    words = np.array([tok[k, i] for _, _, k, i in tuples], np.uint32)
    same("out", got["out"][:len(words)], words)
    assert all(((int(wd) >> 22) & 3) == p for wd, (_, p, _, _) in zip(words[::97], tuples[::97]))
    same("the restatement's own sort", T.stream_words(r), words)


@pytest.mark.parametrize("classes", [0, 2])
def test_hand_over_to_the_packetiser(hip, classes):
    """The entry's out and list_len go to thip_enc_pack_tokens as they are, on the device; the bytes are packref.pack's on the restated
    words."""
    import torch
    from tests import packref as P
    from theora_amd.encoder import pack_tokens, tok_stage
    if classes:
        geo, levels, dcr, cmap = inter_case(2, "random", 3)
        inputs = dict(levels=levels, dcr=dcr, cmap=cmap)
    else:
        geo = T.geometry(*INTER)
        levels, dcq = dc_case(geo, 1)
        inputs = dict(levels=levels, dcq=dcq)
    r = T.restate(geo, classes, want_cover=False, **inputs)
    total = len(r["out"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(a, INT[k]).reshape(-1).view(np.int8 if k == "cmap" else np.int16)).cuda()
           for k, a in inputs.items()}
    n, c = geo.nfrags, T.nchunks(geo.nfrags)
    for k, f in WORDS.items():
        dev[k] = torch.zeros(f(n, c), dtype=torch.int32, device="cuda")
    dev["out"] = torch.zeros(total + PAD, dtype=torch.int32, device="cuda")
    assert tok_stage(INTER[:2], INTER[2], classes, 7, out_cap=total, **{k: t.data_ptr() for k, t in dev.items()}) == 0
    ll = dev["list_len"].cpu().numpy().view(np.uint32).reshape(3, 64).T   # the packetiser's [64][3]
    codes, lens = P.tables("default")
    data, rec = P.pack(r["out"], r["list_len"].reshape(3, 64).T, codes, lens, 4)
    packet = torch.full((rec["bytes"] + 8,), 0x77, dtype=torch.uint8, device="cuda")
    rc, res = pack_tokens(dev["out"].data_ptr(), ll, codes, lens, 3, 4, packet.data_ptr(), rec["bytes"] + 4)
    assert rc == 0 and res == rec
    assert packet[:rec["bytes"]].cpu().numpy().tobytes() == data
