"""The transform-and-quantise kernels of th_encode_* driven directly, through thip_enc_fq_stage: k_enc_intra_fq, k_enc_inter_fq and
k_enc_inter_fq_all, their block-qi forms (enc_fq_bqi of thip_encode_bqi.h) and their masked forms (thip_encode_mask.h), on the caller's
planes, words and tables -- tables, code lengths, scales and decisions no picture sequence reaches.  Every level, dcq, qii, cmap byte and
DC residual is compared for exact equality with tests/fq_stage_ref.py, and the overflow word must be 0; every "this case reaches that
edge" is asserted from the reference inside the test, before the device is asked.  The source always has an odd pitch and an odd base
address; the references come both ways, with a pitch that allows the dword reads of PREV and with one that does not; every output
lies in front of a guard that must come back untouched, and an output the form does not write must come back at its fill.

One edge the kernels' 64-bit D_k cannot reach on 8-bit pictures is stated where it would be tested (test_distortion_at_its_largest)."""
import numpy as np
import pytest

from tests import fq_stage_ref as F
from tests import inter_stage_ref as R
from tests.enc_modes_ref import GOLDEN_MV, GOLDEN_NOMV, INTRA, MV, MV_FOUR, NOMV
from tests.test_gpu_inter_direct import _GUARD, _upload, same
from tests.test_gpu_skip_direct import _bits, _content, _decide, _dequant, _forced

pytestmark = pytest.mark.gpu

OUTS = dict(levels=(128, np.int16), dcq=(2, np.int16), qii=(1, np.uint8), cmap=(1, np.uint8), dcr=(2, np.int16))
FILL = 0x5A


def run(frame, fmt, classes, nqis, planes, dequant, bits=None, prev=None, gold=None, words=None, pic=None, iscale=None, ref_pad=8,
        expect_rc=0, ptrs=None):
    """One call of the entry.  planes: picture-sized planes, rows top first; prev, gold: frame-sized planes in bitstream row order;
    ref_pad: 8 (a pitch and a base that allow dword reads) or 5 (they do not); ptrs: addresses by argument name in place of the ones
    built here (the refusals').  -> dict of what it wrote, `overflow` among it; an output left at its fill comes back as None."""
    import torch
    from theora_amd.encoder import fq_stage
    n = R.geometry(frame[0], frame[1], fmt).nfrags
    keep, kw = [], {}
    k, kw["src"], kw["src_pitch"] = _upload([np.ascontiguousarray(a, np.uint8) for a in planes], 1 if planes[0].shape[1] % 2 == 0 else 2, 1)
    keep += k
    if prev is not None:
        k, kw["prev"], kw["ref_pitch"] = _upload(prev, ref_pad, 0)
        keep += k
    if gold is not None:
        k, kw["gold"], pitch = _upload(gold, ref_pad, 0)
        keep += k
        assert pitch == kw["ref_pitch"]
    if words is not None:
        w = torch.from_numpy(np.ascontiguousarray(words).view(np.uint8).reshape(-1).copy()).cuda()
        keep.append(w)
        kw["words"] = w.data_ptr()
    if iscale is not None:
        t = torch.from_numpy(np.ascontiguousarray(iscale, np.uint16).view(np.uint8).copy()).cuda()
        keep.append(t)
        kw["iscale"] = t.data_ptr()
    outs = {name: torch.full((n * size + _GUARD,), FILL, dtype=torch.uint8, device="cuda") for name, (size, _) in OUTS.items()}
    outs["overflow"] = torch.full((4 + _GUARD,), FILL, dtype=torch.uint8, device="cuda")
    kw.update({name: t.data_ptr() for name, t in outs.items()})
    kw.update(ptrs or {})
    torch.cuda.synchronize()
    rc = fq_stage(frame, fmt, classes, nqis, pic=pic, dequant=dequant, bits=bits, **kw)
    assert rc == expect_rc, rc
    del keep
    res = {}
    for name, t in outs.items():
        size, dt = OUTS.get(name, (0, np.uint32))
        a, nb = t.cpu().numpy(), n * size if size else 4
        assert (a[nb:] == FILL).all(), "%s: written beyond its end" % name
        if (a[:nb] == FILL).all():
            res[name] = None
        else:
            res[name] = a[:nb].view(dt).reshape(n, -1) if name == "levels" else a[:nb].view(dt)
    return res


def check(frame, fmt, classes, nqis, planes, dq, bits=None, d=None, prev=None, gold=None, pic=None, iscale=None, ref_pad=8, want=None):
    """The entry against the reference for the decisions d (pix, mv, bmv or None, words).  -> (the reference's dict, the device's)"""
    fw, fh = frame
    geo = R.geometry(fw, fh, fmt)
    if want is None:
        want = reference(frame, fmt, classes, nqis, planes, dq, bits, d, prev, gold, pic, iscale)
    got = run(frame, fmt, classes, nqis, planes, dq, bits, prev if classes else None, gold if classes == 3 else None,
              d["words"] if classes else None, pic=pic, iscale=iscale, ref_pad=ref_pad)
    written = ["levels", "dcq"] + (["qii"] if nqis else []) + (["cmap", "dcr"] if classes else [])
    for name in OUTS:
        if name in written:
            assert got[name] is not None, "%s: not written" % name
            same(got[name], want[name], name)
        else:
            assert got[name] is None, "%s: written, which this form must not" % name
    assert got["overflow"] is not None and int(got["overflow"][0]) == 0   # (only the token kernel counts into it)
    assert geo.nfrags == len(want["dcq"])
    return want, got


def reference(frame, fmt, classes, nqis, planes, dq, bits=None, d=None, prev=None, gold=None, pic=None, iscale=None):
    fw, fh = frame
    src = R.frame_src(planes, fw, fh, fmt, pic or (0, 0, fw, fh))
    d = d or {}
    return F.stage(R.geometry(fw, fh, fmt), src, classes, nqis, dq, bits, prev, gold, d.get("pix"), d.get("mv"), d.get("bmv"), iscale)


def _mixed(nmbs, classes, seed):
    """Planted decisions: every mode the words of `classes` can carry, in random order, with small vectors."""
    rng = np.random.default_rng(seed)
    modes = [NOMV, INTRA, MV] + ([GOLDEN_NOMV, GOLDEN_MV, MV_FOUR] if classes == 3 else [])
    pix = np.asarray(modes, np.int64)[(rng.permutation(max(nmbs, len(modes))) + seed)[:nmbs] % len(modes)]
    mv = rng.integers(-6, 7, (nmbs, 2))
    mv[~np.isin(pix, (MV, GOLDEN_MV))] = 0
    bmv = rng.integers(-6, 7, (nmbs, 4, 2))
    bmv[pix != MV_FOUR] = 0
    words = R.pack_words8(pix, mv, bmv, np.zeros((nmbs, 2), np.int64)) if classes == 3 else R.pack_words5(pix, mv[:, 0], mv[:, 1])
    return dict(pix=pix, mv=mv, bmv=bmv, words=words)


def _dq(classes, qis):
    """The built-in tables at qis: [n][2][3][64], a key frame's [n][3][64]; qis empty or of one entry for the plain kernel."""
    t = _dequant(qis)
    return t if classes else np.ascontiguousarray(t[:, 0])


def _tables(classes, nlist, seed, scale=(1, 1, 1), s1=None, lo=2, hi=60):
    """Random tables, [nlist][2][3][64] ([nlist][3][64] for a key frame): every step drawn from lo..hi, then times scale[k], times
    7 for the inter tables and times 5 for chroma -- intra and inter, luma and chroma lie far apart --; s1: qis[0]'s step at zig-zag
    index 1 in every table, which sets lambda."""
    rng = np.random.default_rng(seed)
    t = rng.integers(lo, hi + 1, (nlist, 2, 3, 64)).astype(np.int64)
    t *= np.asarray(scale[:nlist], np.int64)[:, None, None, None]
    t[:, 1] *= 7
    t[:, :, 1:] *= 5
    if s1 is not None:
        t[0, :, :, 1] = s1
    t = np.clip(t, 1, 32767).astype(np.uint16)
    return t if classes else np.ascontiguousarray(t[:, 0])


def _rand_bits(seed, lo=0, hi=64):
    return np.random.default_rng(seed).integers(lo, hi + 1, (2, 4, 32)).astype(np.uint8)


def _planted(prev, residual):
    """Picture planes (rows top first) whose residual against PREV at vector 0 is `residual` (three planes, bitstream rows)."""
    out = []
    for a, r in zip(prev, residual):
        s = a.astype(np.int64) + r
        assert s.min() >= 0 and s.max() <= 255
        out.append(np.flipud(s).astype(np.uint8).copy())
    return out


def _checker(shape, amp):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return np.where((yy + xx) & 1, amp, -amp).astype(np.int64)


# ---- sizes and forms ---------------------------------------------------------------------------------------------------------------
# every (classes, nqis, mask) the entry runs: 21
FORMS = [(c, q, m) for c in (0, 2, 3) for q in range(4) for m in (False, True) if q or not m]
# 6 blocks at 4:2:0, a wave mostly idle; one wave; 54 blocks: n ends inside a wave's sixteen; 72 blocks: two work groups; 288 blocks:
# two dclast chunks.  The three small ones take every form, the two large ones a third of them each, every classes among it
SIZES = {(16, 16): FORMS, (32, 16): FORMS, (48, 48): FORMS, (64, 48): FORMS[1::3], (128, 96): FORMS[0::3]}


@pytest.mark.parametrize("frame", list(SIZES), ids=lambda s: "%dx%d" % s)
def test_sizes_formats_and_forms(hip, frame):
    seen, uncoded = set(), 0
    for i, (classes, nqis, mask) in enumerate(SIZES[frame]):
        fmt = 0 if frame == (128, 96) else (0, 2, 3)[(i + frame[0] // 16) % 3]
        geo = R.geometry(frame[0], frame[1], fmt)
        planes, prev, gold = _content(frame[0], frame[1], fmt, 7 * frame[0] + fmt)
        nmbs = (frame[0] // 16) * (frame[1] // 16)
        d = _mixed(nmbs, classes, i) if classes else None
        iscale = np.random.default_rng(i).integers(256, 16384, geo.nfrags).astype(np.uint16) if mask else None
        qis = ([30], [30], [30, 22], [12, 4, 20])[nqis]
        want, _ = check(frame, fmt, classes, nqis, planes, _dq(classes, qis), _bits(("huff", "rand")[i & 1]), d, prev, gold, iscale=iscale,
                        ref_pad=(8, 5)[i & 1])
        seen.add((classes, nqis, mask))
        if nqis > 1 and geo.nfrags > 12:
            assert len(set(want["qii"].tolist())) > 1
        if classes and nmbs >= 6:
            assert {1, 2}.issubset(set(want["cmap"].tolist())) and (classes == 2 or (want["cmap"] == 3).any())
            uncoded += int((want["cmap"] == 0).sum())
    assert {c for c, _, _ in seen} == {0, 2, 3} and (uncoded > 0 or frame[0] * frame[1] < 6 * 256)


assert len(FORMS) == 21 and {f for fs in SIZES.values() for f in fs} == set(FORMS)


@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
def test_a_picture_region_with_odd_offsets(hip, fmt):
    frame, pic = (64, 48), (1, 2, 61, 45)
    from tests import enc_ref
    full, prev, gold = _content(frame[0], frame[1], fmt, 40 + fmt, noise=12)
    planes = [np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in
              zip(full, (enc_ref.chroma_region(pic, fmt, p) for p in range(3)))]
    iscale = np.random.default_rng(fmt).integers(256, 16384, R.geometry(64, 48, fmt).nfrags).astype(np.uint16)
    check(frame, fmt, 0, 0, planes, _dq(0, [30]), pic=pic)
    check(frame, fmt, 0, 3, planes, _dq(0, [30, 22, 38]), _bits("huff"), pic=pic, iscale=iscale)
    for classes in (2, 3):
        d = _decide(frame, fmt, planes, prev, gold, 30, classes == 3, pic)
        want, _ = check(frame, fmt, classes, 2, planes, _dq(classes, [28, 20]), _bits("rand"), d, prev, gold, pic=pic, ref_pad=5,
                        iscale=iscale if classes == 2 else None)
        assert (want["cmap"] != 0).any() and len(set(want["qii"].tolist())) > 1


# ---- equivalences between forms, on the device's own outputs -------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [0, 2, 3])
def test_equivalent_forms_agree(hip, classes):
    frame, fmt = (48, 48), (0, 2, 3)[classes % 3]
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 60 + classes)
    d = _mixed(9, classes, 5) if classes else None
    bits = _bits("huff")
    kw = dict(d=d, prev=prev, gold=gold)
    plain = check(frame, fmt, classes, 0, planes, _dq(classes, [24]), **kw)[1]
    one = check(frame, fmt, classes, 1, planes, _dq(classes, [24]), bits, **kw)[1]
    for name in ("levels", "dcq") + (("cmap", "dcr") if classes else ()):
        same(one[name], plain[name], "a one-entry list against the plain kernel: " + name)
    assert not one["qii"].any()
    # a mask of 2048 everywhere is no mask
    bare = check(frame, fmt, classes, 3, planes, _dq(classes, [24, 16, 32]), bits, **kw)[1]
    unit = check(frame, fmt, classes, 3, planes, _dq(classes, [24, 16, 32]), bits, iscale=np.full(geo.nfrags, 2048, np.uint16), **kw)[1]
    assert len(set(bare["qii"].tolist())) > 1
    for name in ("levels", "dcq", "qii") + (("cmap", "dcr") if classes else ()):
        same(unit[name], bare[name], "a mask of 2048 against none: " + name)
    # three identical tables: every J ties but for the bias, and a tie goes to the lower k
    for lam0 in (False, True):
        t = _dq(classes, [24, 24, 24]).copy()
        if lam0:
            t[..., 1] = 1   # (lambda 0: not even the bias separates them)
        for iscale in (None, np.full(geo.nfrags, 4096, np.uint16)):
            want, got = check(frame, fmt, classes, 3, planes, t, bits, iscale=iscale, **kw)
            assert not got["qii"].any() and (not lam0 or not want["lam"].any())


# ---- tables far apart ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes,fmt", [(0, 0), (2, 3), (3, 0), (3, 2)])
def test_tables_far_apart_and_a_list_out_of_order(hip, classes, fmt):
    """Intra and inter, luma and chroma tables far apart: a wrong table index changes levels.  The list is out of order, coarsest
    first and finest second, with DC steps that differ: a block coded at another qi keeps qis[0]'s DC level."""
    frame = (48, 48)
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 80 + classes + fmt, noise=40)
    d = _mixed(9, classes, 11 + fmt) if classes else None
    dq = _tables(classes, 3, 5, scale=(9, 1, 3), s1=20)
    bits = _rand_bits(3, 1, 24)
    want = reference(frame, fmt, classes, 3, planes, dq, bits, d, prev, gold)
    qii = np.empty(geo.nfrags, np.int64)
    qii[geo.coded_order] = want["qii"]
    moved = np.flatnonzero(qii)
    assert len(moved) and set(qii.tolist()) == {0, 1, 2}
    own_dc = want["lev_k"][qii, np.arange(geo.nfrags), 0]
    assert (own_dc[moved] != want["lev"][moved, 0]).any() and np.array_equal(want["lev"][:, 0], want["lev_k"][0][:, 0])
    if classes:
        # the inter blocks through the intra tables (tab = p for every block) would have other levels
        wrong = dq.copy()
        wrong[:, 1] = wrong[:, 0]
        other = reference(frame, fmt, classes, 3, planes, wrong, bits, d, prev, gold)
        inter = want["qti"] == 1
        assert inter.any() and (~inter).any() and 2 * (other["lev"][inter] != want["lev"][inter]).any(1).sum() > inter.sum()
        assert set(d["pix"].tolist()) == ({NOMV, INTRA, MV} if classes == 2 else {NOMV, INTRA, MV, GOLDEN_NOMV, GOLDEN_MV, MV_FOUR})
    # luma and chroma far apart: the chroma blocks through the luma table would have other levels
    wrong = dq.copy()
    wrong[..., 1:, :] = wrong[..., :1, :]
    other = reference(frame, fmt, classes, 3, planes, wrong, bits, d, prev, gold)
    chroma = geo.plane_of > 0
    assert (other["lev"][chroma] != want["lev"][chroma]).any()
    check(frame, fmt, classes, 3, planes, dq, bits, d, prev, gold, want=want, ref_pad=5)


# ---- the coded flag ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes,mask", [(2, False), (3, False), (3, True)])
def test_the_coded_flag_looks_at_the_chosen_levels(hip, classes, mask):
    """NOMV blocks of two kinds: one whose chosen levels (the second qi's, with qis[0]'s DC) are all zero while the first qi's are not
    -- uncoded --, and one with the DC alone -- coded."""
    frame, fmt = (32, 16), 0
    geo = R.geometry(32, 16, fmt)
    prev = [np.random.default_rng(p).integers(60, 190, s).astype(np.uint8) for p, s in enumerate(((16, 32), (8, 16), (8, 16)))]
    res = [np.zeros(a.shape, np.int64) for a in prev]
    res[0][0:8, 0:8] = _checker((8, 8), 1)       # luma block 0: a zero-mean ripple, something at a fine step and nothing at a coarse one
    res[0][0:8, 8:16] = 20                       # luma block 1: the DC alone
    res[0][8:16, 16:24] = _checker((8, 8), 1)
    res[1][0:8, 0:8] = -9                        # a chroma block with the DC alone
    planes = _planted(prev, res)
    # qis[0]: AC steps of 2 but a DC step of 100 and 16 at index 1 (lambda 80); qis[1]: 60 everywhere
    dq = np.full((2, 2, 3, 64), 2, np.uint16)
    dq[0, :, :, 0], dq[0, :, :, 1], dq[1] = 100, 16, 60
    bits = np.full((2, 4, 32), 12, np.uint8)
    bits[:, :, 0] = 1                            # an EOB is cheap, every other token dear
    iscale = np.full(geo.nfrags, 3000, np.uint16) if mask else None
    d = _forced(2, NOMV, eight=classes == 3)
    want = reference(frame, fmt, classes, 2, planes, dq, bits, d, prev, prev, iscale=iscale)
    ripple, dconly = [0, geo.planes[0]["nhfrags"] + 2], [1, geo.planes[1]["froffset"]]
    for f in ripple:
        assert not want["lev"][f].any() and want["lev_k"][0][f, 1:].any() and want["cmap"][f] == 0
    for f in dconly:
        assert want["lev"][f, 0] != 0 and not want["lev"][f, 1:].any() and want["cmap"][f] == 2
    qii = np.empty(geo.nfrags, np.int64)
    qii[geo.coded_order] = want["qii"]
    assert (qii[ripple] == 1).all()
    assert set(want["cmap"].tolist()) == {0, 2}
    check(frame, fmt, classes, 2, planes, dq, bits, d, prev, prev, iscale=iscale, want=want)


# ---- lambda and its width -------------------------------------------------------------------------------------------------------------
def _choices(want, lam):
    """The choice rule over the reference's D and R with another lambda a block."""
    bias = np.array([0] + [1] * (want["D"].shape[1] - 1), object)
    return np.array([int(np.argmin(want["D"][i] + lam[i] * (want["R"][i] + bias))) for i in range(len(lam))])


@pytest.mark.parametrize("classes", [0, 3])
def test_lambda_zero_is_a_choice_by_distortion(hip, classes):
    """Step 1 at zig-zag index 1 of qis[0]'s tables: lambda = 40 >> 7 = 0.  A scale of 0 does the same to any lambda."""
    frame, fmt = (48, 48), 0
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 90, noise=40)
    d = _mixed(9, classes, 2) if classes else None
    bits = _rand_bits(8)
    for s1, iscale in ((1, None), (1, np.full(geo.nfrags, 40000, np.uint16)), (50, np.zeros(geo.nfrags, np.uint16))):
        dq = _tables(classes, 3, 6, scale=(5, 1, 2), s1=s1)
        want, _ = check(frame, fmt, classes, 3, planes, dq, bits, d, prev, gold, iscale=iscale)
        assert not want["lam"].any() and (want["R"] > 0).all()
        assert np.array_equal(want["qii"], np.argmin(want["D"].astype(np.int64), 1)) and len(set(want["qii"].tolist())) == 3


def _lambda_at_2_32():
    """(s1, iscale) whose lambda_b = (((s1 s1 40) >> 7) iscale + 1024) >> 11 lies at or just above 2^32."""
    for s1 in range(32767, 20724, -1):
        lam = (s1 * s1 * 40) >> 7
        i = -(-((1 << 43) - 1024) // lam)     # the least scale that reaches 2^32
        if i <= 65535 and ((lam * i + 1024) >> 11) - (1 << 32) < 64:
            return s1, i
    raise AssertionError("no such pair")


@pytest.mark.parametrize("classes", [0, 2])
def test_lambda_times_rate_beyond_32_bits(hip, classes):
    """lambda_b lands just above 2^32: kept whole, the rate decides every block; cut to 32 bits, lambda_b would be a few units and the
    distortion would decide.  Then the largest lambda_b there is, with every code 64 bits long."""
    frame, fmt = (48, 48), 0
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 91, noise=40)
    d = _mixed(9, classes, 4) if classes else None
    s1, isc = _lambda_at_2_32()
    dq = _tables(classes, 2, 7, scale=(6, 1), s1=s1)
    bits = _rand_bits(9, 1, 30)
    iscale = np.full(geo.nfrags, isc, np.uint16)
    want = reference(frame, fmt, classes, 2, planes, dq, bits, d, prev, gold, iscale=iscale)
    lam = want["lam"]
    assert all(0 <= int(v) - (1 << 32) < 64 for v in lam) and max(int(v) for v in (lam[:, None] * want["R"]).reshape(-1)) > 1 << 32
    cut = _choices(want, np.array([int(v) & 0xFFFFFFFF for v in lam], object))
    assert (cut != want["qii"]).any() and np.array_equal(_choices(want, lam), want["qii"])
    check(frame, fmt, classes, 2, planes, dq, bits, d, prev, gold, iscale=iscale, want=want)
    dq = _tables(classes, 3, 7, scale=(6, 1, 3), s1=32767)
    bits = np.full((2, 4, 32), 64, np.uint8)
    iscale = np.full(geo.nfrags, 65535, np.uint16)
    want, _ = check(frame, fmt, classes, 3, planes, dq, bits, d, prev, gold, iscale=iscale)
    assert int(want["lam"][0]) == (((32767 * 32767 * 40) >> 7) * 65535 + 1024) >> 11 > 1 << 33
    assert min(int(v) for v in (want["lam"][:, None] * want["R"]).reshape(-1)) > 1 << 38


def test_the_rounding_of_the_scaled_lambda(hip):
    """Scales 0, 1, 2047, 2048, 2049 and 65535 side by side: (lambda iscale + 1024) >> 11 is neither the floor nor the ceiling."""
    frame, fmt, classes = (48, 48), 2, 3
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 92, noise=40)
    d = _mixed(9, classes, 6)
    dq = _tables(classes, 3, 8, scale=(4, 1, 2), s1=29)     # lambda = (841 * 40) >> 7 = 262
    iscale = np.asarray([0, 1, 2047, 2048, 2049, 65535], np.uint16)[np.arange(geo.nfrags) % 6]
    want, _ = check(frame, fmt, classes, 3, planes, dq, _rand_bits(10, 1, 30), d, prev, gold, iscale=iscale)
    isc = iscale[geo.coded_order].astype(np.int64)
    assert (want["lam"][isc == 1] == 0).all() and (want["lam"][isc == 2047] == 262).all() and (want["lam"][isc == 2049] == 262).all()
    for s1, i, lam_b in ((91, 1, 1), (90, 1, 1), (29, 2047 + 8, 263)):   # (s1 s1 40) >> 7 = 2587, 2531: above 1024 a unit scale keeps one
        assert F.S.block_lambda([0, s1], i) == lam_b
    dq = _tables(classes, 3, 8, scale=(4, 1, 2), s1=91)
    want, _ = check(frame, fmt, classes, 3, planes, dq, _rand_bits(10, 1, 30), d, prev, gold, iscale=iscale)
    assert (want["lam"][isc == 1] == 1).all() and (want["lam"][isc == 0] == 0).all()


def test_distortion_at_its_largest(hip):
    """A step of 32767 everywhere on +-255 checkerboard residuals: every level is zero and D_k is the block's whole energy, the
    largest any residual searched gives (checkerboards, random +-255, separable and three-valued patterns, 80 000 blocks: the int16
    transform wraps on them and tops out at 6.7e7, under 2^27).  D_k past 2^32, which the kernels' 64-bit sums would hold, is not
    reached through 8-bit pixels by any content known here, so that crossing is not asserted; this is the case nearest to it."""
    frame, fmt = (32, 16), 3
    geo = R.geometry(32, 16, fmt)
    prev = [np.where(_checker(s, 1) > 0, 255, 0).astype(np.uint8) for s in ((16, 32),) * 3]
    planes = [np.flipud(255 - a).copy() for a in prev]
    dq = np.full((2, 2, 3, 64), 32767, np.uint16)
    dq[1] = 32000
    d = _forced(2, NOMV)
    want, _ = check(frame, fmt, 3, 2, planes, dq, _rand_bits(12, 1, 30), d, prev, prev, iscale=np.full(geo.nfrags, 65535, np.uint16))
    top = max(int(v) for v in want["D"].reshape(-1))
    assert 1 << 25 < top < 1 << 27 and not want["lev"].any() and not want["cmap"].any()


# ---- levels beyond +-580 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [0, 2])
def test_levels_beyond_580_go_out_whole(hip, classes):
    """Steps 1..3 on checkerboards of several swings: levels beyond the largest token's range go out unclamped, count in R_k as
    token 22 does (planted 64 bits long, every other token at most 10), and leave the overflow word alone.  The scales make lambda_b
    0, 2 and 64 from block to block, so that the distortion decides some blocks and the rate others."""
    frame, fmt = (32, 16), 0
    geo = R.geometry(32, 16, fmt)
    swing = [np.kron(np.asarray([[127, 100, 60, 30], [30, 60, 100, 127]])[:s[0] // 8, :s[1] // 8], np.ones((8, 8), np.int64))
             for s in ((16, 32), (8, 16), (8, 16))]
    board = [128 + np.where(_checker(a.shape, 1) > 0, a, -a) for a in swing]
    if classes:
        prev = [(255 - b).astype(np.uint8) for b in board]      # (NOMV against the inverse: twice the swing)
        planes = [np.flipud(b).astype(np.uint8).copy() for b in board]
    else:
        prev, planes = None, [np.flipud(b).astype(np.uint8).copy() for b in board]
    dq = np.empty((3, 2, 3, 64), np.uint16)
    dq[0], dq[1], dq[2] = 3, 1, 2
    dq = dq if classes else np.ascontiguousarray(dq[:, 0])
    bits = _rand_bits(13, 1, 10)
    bits[:, :, 22] = 64
    iscale = np.asarray([0, 2048, 65535], np.uint16)[np.arange(geo.nfrags) % 3]
    d = _forced(2, NOMV, eight=False) if classes else None
    want = reference(frame, fmt, classes, 3, planes, dq, bits, d, prev, iscale=iscale)
    assert np.abs(want["levels"][:, 1:]).max() > 580 and len(set(want["qii"].tolist())) > 1
    Rk = np.empty((geo.nfrags, 3), object)
    Rk[geo.coded_order] = want["R"]
    n22 = (np.abs(want["lev_k"][:, :, 1:]) >= 69).sum(2).T        # token 22: 69 and beyond
    beyond = (np.abs(want["lev_k"][:, :, 1:]) > 580).sum(2).T
    assert (beyond > 0).any() and (Rk >= 64 * n22).all() and (Rk <= 64 * n22 + 10 * 64).all()
    check(frame, fmt, classes, 3, planes, dq, bits, d, prev, iscale=iscale, want=want)


# ---- bits tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [0, 3])
def test_bits_tables(hip, classes):
    """Random lengths 0..64; the all-zero table (R = 0: the distortion and the bias alone); luma and chroma tables swapped."""
    frame, fmt = (48, 48), 3
    geo = R.geometry(48, 48, fmt)
    planes, prev, gold = _content(48, 48, fmt, 95, noise=40)
    d = _mixed(9, classes, 8) if classes else None
    dq = _tables(classes, 3, 10, scale=(3, 1, 2), s1=10)
    check(frame, fmt, classes, 3, planes, dq, _rand_bits(14), d, prev, gold)
    want, _ = check(frame, fmt, classes, 3, planes, dq, np.zeros((2, 4, 32), np.uint8), d, prev, gold)
    assert not want["R"].any() and want["lam"].all() and len(set(want["qii"].tolist())) > 1
    bits = _rand_bits(15, 1, 6)
    bits[1] += 40
    a, _ = check(frame, fmt, classes, 3, planes, dq, bits, d, prev, gold)
    b, _ = check(frame, fmt, classes, 3, planes, dq, bits[::-1].copy(), d, prev, gold)
    assert (a["qii"] != b["qii"]).any()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip):
    """The entry's own refusals, on real buffers: the code, and every output still at its fill."""
    frame, fmt = (32, 16), 0
    planes, prev, gold = _content(32, 16, fmt, 3)
    d8, d5 = _forced(2, MV, (2, 2)), _forced(2, MV, (2, 2), eight=False)
    EFAULT, EINVAL = -1, -10
    bits = _bits("huff")

    def refused(rc, classes, nqis, words=None, **kw):
        use_gold = kw.pop("use_gold", classes == 3)
        dq = kw.pop("dequant", _dq(classes if classes in (0, 2, 3) else 2, [30, 22, 38][:max(min(nqis, 3), 1)]))
        got = run(frame, fmt, classes, nqis, planes, dq, kw.pop("bits", bits), None if kw.pop("no_prev", False) else prev,
                  gold if use_gold else None, words, expect_rc=rc, ptrs=kw)
        assert all(v is None for v in got.values()), [k for k, v in got.items() if v is not None]

    some = np.full(12, 2048, np.uint16)
    refused(EINVAL, 3, -1, d8["words"])
    refused(EINVAL, 3, 4, d8["words"], dequant=_dq(3, [30, 22, 38]))
    refused(EINVAL, 1, 1, d5["words"])
    refused(EINVAL, 4, 1, d8["words"])
    refused(EINVAL, 2, 1, d5["words"], use_gold=True)     # gold with classes below 3
    refused(EINVAL, 0, 1, use_gold=True)
    refused(EFAULT, 3, 1, d8["words"], use_gold=False)
    refused(EFAULT, 2, 1, None)                           # no words
    refused(EFAULT, 2, 1, d5["words"], cmap=None)
    refused(EFAULT, 2, 1, d5["words"], qii=None)
    refused(EFAULT, 0, 2, levels=None)
    refused(EFAULT, 0, 2, dcq=None)
    refused(EFAULT, 0, 2, bits=None)
    refused(EFAULT, 0, 2, dequant=None)
    refused(EFAULT, 2, 0, d5["words"], no_prev=True)
    for classes, nqis, words in ((0, 0, None), (2, 0, d5["words"]), (3, 0, d8["words"])):
        got = run(frame, fmt, classes, nqis, planes, _dq(classes, [30]), None, prev, gold if classes == 3 else None, words,
                  iscale=some, expect_rc=EINVAL)                     # scales without a list
        assert all(v is None for v in got.values())
    t = _dq(2, [30, 22]).copy()
    t[1, 1, 2, 63] = 0
    refused(EINVAL, 2, 2, d5["words"], dequant=t)
    t = _dq(0, [30]).astype(np.int64)
    t[0, 0, 0] = 32768
    refused(EINVAL, 0, 0, dequant=t)
    b = bits.copy()
    b[1, 3, 31] = 65
    refused(EINVAL, 0, 1, bits=b)
    import torch
    spare = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    for name, off in (("levels", 8), ("dcq", 1), ("dcr", 1), ("overflow", 2), ("iscale", 1)):
        refused(EINVAL, 3, 1, d8["words"], **{name: spare.data_ptr() + off})
    w = torch.from_numpy(np.concatenate([np.zeros(8, np.uint8), d8["words"].view(np.uint8).reshape(-1)])).cuda()
    got = run(frame, fmt, 3, 1, planes, _dq(3, [30]), bits, prev, gold, None, expect_rc=EINVAL, ptrs=dict(words=w.data_ptr() + 8))
    assert all(v is None for v in got.values())
    assert (spare.cpu().numpy() == FILL).all()
    # and the same request with nothing wrong runs
    check(frame, fmt, 3, 1, planes, _dq(3, [30]), bits, d8, prev, gold)
