"""The level choice of th_encode_* driven directly, through thip_enc_rdq_stage: the launch of thip_encode_rdq.h on the caller's planes,
words, tables and LEVELS.  Every level and every block's jbefore, jafter and rate is compared for exact equality with
tests/enc_rdq_ref.py; every "this case reaches that edge" is asserted from the reference inside the test.  The source always has an
odd pitch and an odd base address; every output lies in front of a guard that must come back untouched."""
import functools

import numpy as np
import pytest

import oracle
from tests import enc_modes_ref as M
from tests import enc_ref
from tests import enc_rdq_ref as Q
from tests import enc_skip_ref as S
from tests import inter_stage_ref as R
from tests.packref import EXTRA_BITS
from tests.test_gpu_inter_direct import _GUARD, _upload, same

pytestmark = pytest.mark.gpu

OUTS = dict(jbefore=np.int64, jafter=np.int64, rate=np.int64)


@functools.lru_cache(None)
def _setup():
    from theora_amd.encoder import Encoder
    e = Encoder(16, 16, 0, 32)
    s = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    return s


def _dequant(qis):
    """[nqis][2][3][64] zig-zag."""
    return np.stack([R.tables_qi(_setup(), q) for q in qis]).astype(np.uint16)


def _bits(kind):
    if kind == "huff":
        return S.stage_bits(_setup(), (5, 12))
    if kind == "flat":   # every token the same: ties everywhere
        return np.full((2, 4, 32), 7, np.uint8)
    return (np.random.default_rng(17).integers(1, 20, (2, 4, 32)) + np.asarray(EXTRA_BITS)[None, None, :]).astype(np.uint8)


def run(frame, fmt, classes, nqis, planes, prev, gold, words, dequant, bits, levels, qii, cmap, w, pic=None, lam=-1, iscale=None):
    """One call of the entry.  planes: picture-sized planes, rows top first; prev, gold: frame-sized planes in bitstream row order (None
    with classes 0); levels [n, 64], qii [n] or None (coded order), cmap [n] raster or None.  -> dict of what it wrote."""
    import torch
    from theora_amd.encoder import rdq_stage
    n = R.geometry(frame[0], frame[1], fmt).nfrags
    keep, kw = [], {}
    k, kw["src"], kw["src_pitch"] = _upload([np.ascontiguousarray(a, np.uint8) for a in planes], 1 if planes[0].shape[1] % 2 == 0 else 2, 1)
    keep += k
    if classes:
        k, kw["prev"], kw["ref_pitch"] = _upload(prev, 5, 0)
        keep += k
    if classes == 3:
        k, kw["gold"], _ = _upload(gold, 5, 0)
        keep += k

    def dev(a, dt):
        t = torch.from_numpy(np.concatenate([np.ascontiguousarray(a, dt).view(np.uint8).reshape(-1), np.full(_GUARD, 0x5A, np.uint8)])).cuda()
        keep.append(t)
        return t
    if classes:
        kw["words"] = dev(words, np.asarray(words).dtype).data_ptr()
        kw["cmap"] = dev(cmap, np.uint8).data_ptr()
    if qii is not None:
        kw["qii"] = dev(qii, np.uint8).data_ptr()
    if iscale is not None:
        kw["iscale"] = dev(iscale, np.uint16).data_ptr()
    lv = dev(levels, np.int16)
    outs = {name: torch.full((n * 8 + _GUARD,), 0x5A, dtype=torch.uint8, device="cuda") for name in OUTS}
    torch.cuda.synchronize()
    rc = rdq_stage(frame, fmt, classes, nqis, w, pic=pic, lam=lam, dequant=dequant, bits=bits, levels=lv.data_ptr(),
                   **{name: t.data_ptr() for name, t in outs.items()}, **kw)
    assert rc == 0, rc
    res = {}
    for name, t in dict(outs, levels=lv).items():
        a, size = t.cpu().numpy(), n * (128 if name == "levels" else 8)
        assert (a[size:] == 0x5A).all(), "%s: written beyond its end" % name
        res[name] = a[:size].view(np.int16).reshape(n, 64) if name == "levels" else a[:size].view(np.int64)
    return res


def check(frame, fmt, classes, planes, prev, gold, d, qis, bits, levels, qii, cmap, w, pic=None, lam=-1, iscale=None):
    """The entry against the restatement.  d: the macro blocks' decisions (pix, mv, bmv, words), None with classes 0.  -> the
    restatement's dict"""
    fw, fh = frame
    geo = R.geometry(fw, fh, fmt)
    src = R.frame_src(planes, fw, fh, fmt, pic or (0, 0, fw, fh))
    dq = _dequant(qis)
    d = d or {}
    want = Q.stage(geo, src, prev, gold if classes == 3 else None, classes, d.get("pix"), d.get("mv"), d.get("bmv"), dq, bits, levels, qii,
                   cmap, w, iscale, None if lam < 0 else lam)
    got = run(frame, fmt, classes, len(qis), planes, prev, gold, d.get("words"), dq, bits, levels, qii, cmap, w, pic=pic, lam=lam,
              iscale=iscale)
    for name in ("levels",) + tuple(OUTS):
        same(got[name], want[name], name)
    lv = np.asarray(levels, np.int64)
    assert (want["levels"][:, 0] == lv[:, 0]).all() and (want["levels"][lv == 0] == 0).all()   # the DC and the zeros stay
    if classes:
        unc = np.asarray(cmap)[geo.coded_order] == 0
        assert (want["levels"][unc] == lv[unc]).all() and not want["jbefore"][unc].any()
    return want


def _content(fw, fh, fmt, seed, noise=10, pic=None):
    """(picture planes rows top first, prev, gold in bitstream rows): crops of one image; PREV the same crop a pixel off under noise."""
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    rng = np.random.default_rng(seed)
    big = [enc_ref.content("natural", (fh + 32, fw + 32), seed + p) for p in range(3)]

    def crop(dx, dy, amp):
        out = []
        for p in range(3):
            sx, sy = (hd, vd) if p else (0, 0)
            a = big[p][16 + dy:16 + dy + fh:1 + sy, 16 + dx:16 + dx + fw:1 + sx].astype(np.int64)
            out.append(np.clip(a + rng.integers(-amp, amp + 1, a.shape), 0, 255).astype(np.uint8))
        return out
    full = crop(0, 0, 0)
    if pic is not None:
        full = [np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in
                zip(full, (enc_ref.chroma_region(pic, fmt, p) for p in range(3)))]
    return full, [np.flipud(a).copy() for a in crop(1, 0, noise)], [np.flipud(a).copy() for a in crop(2, 1, 6)]


def _honest(frame, fmt, classes, planes, prev, gold, qis, bits, seed, pic=None):
    """Levels, cmap and the decisions as a frame's quantising kernels would leave them, under a planted qii: the skip restatement's
    at lambda 0 for an inter frame, the plain quantiser's for a key frame."""
    fw, fh = frame
    geo = R.geometry(fw, fh, fmt)
    src = R.frame_src(planes, fw, fh, fmt, pic or (0, 0, fw, fh))
    dq = _dequant(qis)
    rng = np.random.default_rng(seed)
    if classes:
        d = R.decide8(M.search_all(src[0], prev[0], gold[0]), 30) if classes == 3 else R.decide5(R.search(src[0], prev[0]), 30)
        st = S.stage(geo, src, prev, gold if classes == 3 else None, d["pix"], d["mv"], d.get("bmv"), dq, bits, lam_fix=0)
        return d, st["levels"], rng.integers(0, len(qis), geo.nfrags).astype(np.uint8), st["cmap"]   # (a planted qii)
    qii = rng.integers(0, len(qis), geo.nfrags).astype(np.uint8)
    lev = np.zeros((geo.nfrags, 64), np.int16)
    r8 = np.arange(8)
    for k, f in enumerate(geo.coded_order):
        p = int(geo.plane_of[f])
        g = geo.planes[p]
        loc = f - g["froffset"]
        Y, X = (loc // g["nhfrags"]) * 8 + r8[:, None], (loc % g["nhfrags"]) * 8 + r8[None, :]
        c = oracle.fdct8x8_batch((src[p][Y, X] - 128).reshape(1, 64).astype(np.int16))
        lev[k] = oracle.quantize_batch(c, dq[qii[k], 0, p])[0][0]
        lev[k, 0] = oracle.quantize_batch(c, dq[0, 0, p])[0][0][0]
    return None, lev, qii, None


GEOMETRY = [((16, 16), 0), ((48, 48), 0), ((32, 32), 2), ((32, 32), 3), ((96, 80), 0)]


@pytest.mark.parametrize("classes", [0, 2, 3])
@pytest.mark.parametrize("frame,fmt", GEOMETRY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sizes_formats_classes_and_lists(hip, frame, fmt, classes):
    """One macro block; sixteen blocks that straddle luma and chroma; 4:2:2 and 4:4:4; several work groups and a short last wave.
    Each with a one-, two- and three-entry qi list, with and without masking's scales, at weights 1, 16 and 64."""
    planes, prev, gold = _content(frame[0], frame[1], fmt, 7 * frame[0] + fmt + classes)
    geo = R.geometry(frame[0], frame[1], fmt)
    iscale = np.random.default_rng(3).integers(512, 8192, geo.nfrags).astype(np.uint16)
    changed = kept = 0
    for qis, bits, masked, w in (([30], "huff", False, 16), ([30, 22], "rand", True, 64), ([24, 16, 32], "huff", False, 1)):
        d, lev, qii, cmap = _honest(frame, fmt, classes, planes, prev, gold, qis, _bits(bits), 5)
        if classes and frame != (16, 16):
            # uncoded blocks, whatever their levels: every seventh of the coded order, and all the luma of the first macro block,
            # whose chroma is then INTER_NOMV whatever its word says
            cmap = np.asarray(cmap).copy()
            cmap[geo.coded_order[::7]] = 0
            cmap[[0, 1, geo.planes[0]["nhfrags"], geo.planes[0]["nhfrags"] + 1]] = 0
        if len(qis) > 1 and frame != (16, 16):
            assert len(set(np.asarray(qii).tolist())) > 1
        want = check(frame, fmt, classes, planes, prev, gold, d, qis, _bits(bits), lev, qii if len(qis) > 1 else None, cmap, w,
                     iscale=iscale if masked else None)
        diff = (want["levels"] != lev).any(1)
        changed += int(diff.sum())
        kept += int((~diff & (lev[:, 1:] != 0).any(1)).sum())
        if classes and frame != (16, 16):
            assert (np.asarray(cmap) == 0).any() and (np.asarray(cmap) != 0).any()
    assert changed > 0 and (kept > 0 or frame == (16, 16))   # (six blocks may all change)


@pytest.mark.parametrize("classes", [0, 3])
def test_a_picture_region_with_odd_offsets(hip, classes):
    frame, fmt, pic = (48, 32), 0, (5, 3, 37, 25)
    planes, prev, gold = _content(48, 32, fmt, 41, pic=pic)
    d, lev, qii, cmap = _honest(frame, fmt, classes, planes, prev, gold, [28, 20], _bits("huff"), 9, pic=pic)
    want = check(frame, fmt, classes, planes, prev, gold, d, [28, 20], _bits("huff"), lev, qii, cmap, 16, pic=pic)
    assert (want["levels"] != lev).any()


def _patterns():
    """Planted blocks: name -> {zig-zag index: level}."""
    pat = {"all +-1": {z: (1 if z % 3 else -1) for z in range(1, 64)},
           "+-1 and +-2": {z: ((1, -2, -1, 2)[z % 4]) for z in range(1, 64)},
           "last at 62": {2: 3, 62: -1}, "last at 63": {1: -2, 63: 1}, "only 63": {63: 2}}
    for run in (5, 6, 9, 10, 17, 18):          # +-1 behind a run of `run` zeros: both sides of the combined tokens' edges
        pat["+-1 after %d" % run] = {1: 4, 2 + run: -1, 4 + run: 1}
    for run in (1, 3, 4):                      # +-2, +-3 behind short runs
        pat["2, 3 after %d" % run] = {1: 1, 2 + run: 2, 3 + 2 * run: -3, 4 + 3 * run: 1}
    for run in (8, 9):                         # the short and the long zero run
        pat["zeros %d" % run] = {1: -5, 2 + run: 7, 3 + 2 * run: 2}
    for m in (2, 3, 6, 7, 8, 9, 12, 13, 20, 21, 36, 37, 68, 69):   # both sides of every value-token category edge
        pat["magnitude %d" % m] = {1: m, 3: -m, 4: 1, 9: -m}
    for z in (5, 6, 14, 15, 27, 28):           # both sides of the Huffman-group edges
        pat["group edge %d" % z] = {z: 1, z + 1: -2, z + 3: 1}
    return pat


@pytest.mark.parametrize("bits,lam,w", [("huff", -1, 16), ("huff", -1, 64), ("rand", 0, 16), ("flat", 300, 16), ("rand", 1 << 40, 1),
                                         ("huff", 1 << 40, 64), ("flat", -1, 5), ("flat", 1 << 40, 16)],
                         ids=["own-16", "own-64", "zero", "flat", "huge-1", "huge-64", "flat-own-5", "flat-huge"])
def test_planted_levels(hip, bits, lam, w):
    """Every pattern on a luma and on a chroma block of a key frame, the coefficients close to the planted levels: the heaviest block,
    the edges of every token category, run length and Huffman group, a last level at 62 and at 63; lambda 0, a block's own, 2^40;
    a bits table that ties."""
    frame, fmt, qis = (48, 48), 3, [30]
    geo = R.geometry(48, 48, fmt)
    planes, _, _ = _content(48, 48, fmt, 3)
    _, lev, _, _ = _honest(frame, fmt, 0, planes, None, None, qis, _bits(bits), 1)
    pat = _patterns()
    assert 2 * len(pat) <= geo.nfrags
    for i, (name, lv) in enumerate(pat.items()):
        for k in (i, geo.nfrags - 1 - i):      # coded order: a luma block, a chroma block
            lev[k, 1:] = 0
            for z, v in lv.items():
                lev[k, z] = v
    want = check(frame, fmt, 0, planes, None, None, None, qis, _bits(bits), lev, None, None, w, lam=lam)
    if lam == 0:
        assert (want["levels"] == lev).all() and (want["jbefore"] == want["jafter"]).all()
    else:
        assert (want["jafter"] <= want["jbefore"]).all() and (want["levels"] != lev).any()
    if lam == 1 << 40:
        assert (np.abs(want["levels"][1]) >= (np.abs(lev[1]) >= 2)).all()   # a level |l| >= 2 never becomes 0
        if bits == "flat":   # every token the same price and the error next to nothing: the EOB alone is the one cheapest block
            assert not want["levels"][0, 1:].any() and int(want["rate"][0]) == 7


def test_planted_levels_on_an_inter_frame(hip):
    """The patterns on coded and uncoded blocks of an eight-mode inter frame with a three-entry list: uncoded blocks come back as they
    went, whatever they hold."""
    frame, fmt, qis = (48, 48), 0, [30, 22, 38]
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 13)
    d, lev, qii, cmap = _honest(frame, fmt, 3, planes, prev, gold, qis, _bits("huff"), 2)
    lev = lev.copy()
    for i, lv in enumerate(list(_patterns().values())[:geo.nfrags]):
        lev[i, 1:] = 0
        for z, v in lv.items():
            lev[i, z] = v
    cm = np.asarray(cmap).copy()
    cm[geo.coded_order[::5]] = 0    # planted uncoded blocks, some of them whole macro blocks' luma
    assert (cm == 0).any() and (cm != 0).any()
    want = check(frame, fmt, 3, planes, prev, gold, d, qis, _bits("huff"), lev, qii, cm, 16)
    assert (want["levels"] != lev).any()


def test_lambda_at_below_and_above_one_blocks_equality(hip):
    """One level +-1 at z in an otherwise empty block, lambda planted so that keeping it and dropping it cost the same: it stays at
    the equality (a tie keeps the coefficient) and one below, and goes one above."""
    frame, fmt, qis, bits = (32, 32), 0, [30], _bits("huff")
    geo = R.geometry(32, 32, fmt)
    planes, _, _ = _content(32, 32, fmt, 23)
    src = R.frame_src(planes, 32, 32, fmt, (0, 0, 32, 32))
    dq = _dequant(qis)
    fb = Q.full_bits((np.asarray(bits, np.int64)[0] - np.asarray(EXTRA_BITS)[None, :]).tolist())
    hit = None
    for k in range(16):   # luma blocks
        f = int(geo.coded_order[k])
        Y, X = (f // 4) * 8 + np.arange(8)[:, None], (f % 4) * 8 + np.arange(8)[None, :]
        c = oracle.fdct8x8_batch((src[0][Y, X] - 128).reshape(1, 64).astype(np.int16))[0].astype(np.int64)
        for z in range(1, 64):
            s = int(dq[0, 0, 0, z])
            l = 1 if c[z] >= 0 else -1
            dd = int(c[z]) ** 2 - (int(c[z]) - l * s) ** 2
            dr = Q.value_bits(l, z, 1, fb) + (fb[Q.group(z + 1)][0] if z < 63 else 0) - fb[0][0]
            if dd > 0 and dr > 0 and dd % dr == 0 and dd // dr > 1:
                hit = (k, z, l, dd // dr)
                break
        if hit:
            break
    assert hit
    k, z, l, lam = hit
    lev = np.zeros((geo.nfrags, 64), np.int16)
    lev[k, z] = l
    got = {dl: check(frame, fmt, 0, planes, None, None, None, qis, bits, lev, None, None, 16, lam=lam + dl) for dl in (-1, 0, 1)}
    assert [int(got[dl]["levels"][k, z]) for dl in (-1, 0, 1)] == [l, l, 0]
    assert int(got[0]["jbefore"][k]) == int(got[0]["jafter"][k]) and int(got[1]["jafter"][k]) < int(got[1]["jbefore"][k])
