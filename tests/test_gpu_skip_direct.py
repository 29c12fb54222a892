"""The skip decision of th_encode_* driven directly, through thip_enc_skip_stage: the two launches of thip_encode_skip.h (the luma
blocks, then the chroma blocks) on the caller's planes, words and tables.  Every level, cmap byte, qii, flag, D_code, R and D_skip is
compared for exact equality with tests/enc_skip_ref.py; every "this case reaches that edge" is asserted from the reference inside the
test.  The source always has an odd pitch and an odd base address; the references come both ways, with a pitch that allows the dword
reads of PREV and with one that does not; every output lies in front of a guard that must come back untouched."""
import functools

import numpy as np
import pytest

from tests import enc_modes_ref as M
from tests import enc_ref
from tests import enc_skip_ref as S
from tests import inter_stage_ref as R
from tests.enc_modes_ref import GOLDEN_MV, INTRA, MV, MV_FOUR, NOMV
from tests.packref import EXTRA_BITS
from tests.test_gpu_inter_direct import _GUARD, _upload, same

pytestmark = pytest.mark.gpu

OUTS = dict(levels=(128, np.int16), dcq=(2, np.int16), qii=(1, np.uint8), cmap=(1, np.uint8), skf=(1, np.uint8), dcode=(8, np.int64),
            rate=(8, np.int64), dskip=(8, np.int64))


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
    return (np.random.default_rng(17).integers(1, 20, (2, 4, 32)) + np.asarray(EXTRA_BITS)[None, None, :]).astype(np.uint8)


def run(frame, fmt, classes, nqis, planes, prev, gold, words, dequant, bits, pic=None, lam=-1, iscale=None, ref_pad=8):
    """One call of the entry.  planes: picture-sized planes, rows top first; prev, gold: frame-sized planes in bitstream row order;
    ref_pad: 8 (a pitch and a base that allow dword reads) or 5 (they do not).  -> dict of what it wrote."""
    import torch
    from theora_amd.encoder import skip_stage
    geo = R.geometry(frame[0], frame[1], fmt)
    n = geo.nfrags
    keep, kw = [], {}
    k, kw["src"], kw["src_pitch"] = _upload([np.ascontiguousarray(a, np.uint8) for a in planes], 1 if planes[0].shape[1] % 2 == 0 else 2, 1)
    keep += k
    k, kw["prev"], kw["ref_pitch"] = _upload(prev, ref_pad, 0)
    keep += k
    if classes == 3:
        k, kw["gold"], pitch = _upload(gold, ref_pad, 0)
        keep += k
        assert pitch == kw["ref_pitch"]
    w = torch.from_numpy(np.ascontiguousarray(words).view(np.uint8).reshape(-1).copy()).cuda()
    keep.append(w)
    if iscale is not None:
        t = torch.from_numpy(np.ascontiguousarray(iscale, np.uint16).view(np.uint8).copy()).cuda()
        keep.append(t)
        kw["iscale"] = t.data_ptr()
    outs = {}
    for name, (size, _) in OUTS.items():
        outs[name] = torch.full((n * size + _GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        kw[name] = outs[name].data_ptr()
    torch.cuda.synchronize()
    rc = skip_stage(frame, fmt, classes, nqis, pic=pic, lam=lam, words=w.data_ptr(), dequant=dequant, bits=bits, **kw)
    assert rc == 0, rc
    del keep
    res = {}
    for name, (size, dt) in OUTS.items():
        a = outs[name].cpu().numpy()
        assert (a[n * size:] == 0x5A).all(), "%s: written beyond its end" % name
        res[name] = a[:n * size].view(dt).reshape(n, -1) if name == "levels" else a[:n * size].view(dt)
    return res


def check(frame, fmt, planes, prev, gold, d, nqis_qis, bits, pic=None, lam=-1, iscale=None, ref_pad=8):
    """The entry against the restatement for the decisions d (pix, mv, bmv or None, words).  -> the restatement's dict"""
    fw, fh = frame
    geo = R.geometry(fw, fh, fmt)
    src = R.frame_src(planes, fw, fh, fmt, pic or (0, 0, fw, fh))
    dq = _dequant(nqis_qis)
    classes = 3 if np.asarray(d["words"]).ndim == 2 else 2
    want = S.stage(geo, src, prev, gold if classes == 3 else None, d["pix"], d["mv"], d.get("bmv"), dq, bits, iscale,
                   None if lam < 0 else lam)
    got = run(frame, fmt, classes, len(nqis_qis), planes, prev, gold, d["words"], dq, bits, pic=pic, lam=lam, iscale=iscale,
              ref_pad=ref_pad)
    for name in OUTS:
        same(got[name], want[name], name)
    return want


def _content(fw, fh, fmt, seed, noise=24, shift=(0, 0)):
    """(picture planes rows top first, prev, gold in bitstream rows): crops of one image; PREV the same crop moved by `shift` under
    noise that grows from nothing at one corner to +-`noise` at the opposite one, so that the rules before the test leave some blocks
    uncoded, the test leaves some out and others are coded; GOLD moved further."""
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    rng = np.random.default_rng(seed)
    big = [enc_ref.content("natural", (fh + 32, fw + 32), seed + p) for p in range(3)]

    def crop(dx, dy, amp):
        out = []
        for p in range(3):
            sx, sy = (hd, vd) if p else (0, 0)
            a = big[p][16 + dy:16 + dy + fh:1 + sy, 16 + dx:16 + dx + fw:1 + sx].astype(np.int64)
            yy, xx = np.mgrid[0:a.shape[0], 0:a.shape[1]]
            grow = ((xx + yy) * amp) // (a.shape[0] + a.shape[1])
            out.append(np.clip(a + rng.integers(-grow, grow + 1), 0, 255).astype(np.uint8))
        return out
    return crop(0, 0, 0), [np.flipud(a).copy() for a in crop(shift[0], shift[1], noise)], [np.flipud(a).copy() for a in crop(2, 1, 6)]


def _decide(frame, fmt, planes, prev, gold, lam, eight, pic=None):
    src = R.frame_src(planes, frame[0], frame[1], fmt, pic or (0, 0, frame[0], frame[1]))
    if eight:
        return R.decide8(M.search_all(src[0], prev[0], gold[0]), lam)
    return R.decide5(R.search(src[0], prev[0]), lam)


def _forced(nmbs, mode, vec=(0, 0), bmv=None, eight=True):
    pix, mv = np.full(nmbs, mode, np.int64), np.tile(np.asarray(vec, np.int64), (nmbs, 1))
    b = np.zeros((nmbs, 4, 2), np.int64) if bmv is None else np.tile(np.asarray(bmv, np.int64), (nmbs, 1, 1))
    words = R.pack_words8(pix, mv, b, np.zeros((nmbs, 2), np.int64)) if eight else R.pack_words5(pix, mv[:, 0], mv[:, 1])
    return dict(pix=pix, mv=mv, bmv=b, words=words)


SIZES = [(16, 16), (32, 16), (48, 48)]   # one macro block; one wave; 36 luma blocks: the chroma launch starts inside a wave's sixteen


@pytest.mark.parametrize("eight", [False, True], ids=["five", "eight"])
@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
@pytest.mark.parametrize("frame", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_formats_words_and_lists(hip, frame, fmt, eight):
    planes, prev, gold = _content(frame[0], frame[1], fmt, 5 * frame[0] + fmt)
    geo = R.geometry(frame[0], frame[1], fmt)
    iscale = np.random.default_rng(3).integers(512, 8192, geo.nfrags).astype(np.uint16)
    d = _decide(frame, fmt, planes, prev, gold, 30, eight)
    skipped = coded = 0
    for qis, bits, masked, pad in (([30], "huff", False, 8), ([30, 22], "rand", True, 5), ([30, 22, 38], "huff", False, 5),
                                   ([12, 4, 20], "rand", True, 8)):
        want = check(frame, fmt, planes, prev, gold, d, qis, _bits(bits), iscale=iscale if masked else None, ref_pad=pad)
        skipped += int(want["skf"].sum())
        coded += int((want["cmap"] != 0).sum())
        if len(qis) > 1 and frame != (16, 16):
            assert len(set(want["qii"].tolist())) > 1
    assert skipped > 0 and coded > 0


@pytest.mark.parametrize("eight", [False, True], ids=["five", "eight"])
@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
def test_a_picture_region_with_odd_offsets(hip, fmt, eight):
    frame, pic = (48, 32), (5, 3, 37, 25)
    full, prev, gold = _content(frame[0], frame[1], fmt, 40 + fmt, noise=12)
    planes = [np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in
              zip(full, (enc_ref.chroma_region(pic, fmt, p) for p in range(3)))]
    d = _decide(frame, fmt, planes, prev, gold, 30, eight, pic)
    want = check(frame, fmt, planes, prev, gold, d, [28, 20], _bits("huff"), pic=pic, ref_pad=5)
    assert want["skf"].any() and (want["cmap"] != 0).any()


def test_lambda_at_below_and_above_the_equality(hip):
    """lambda planted so that D_skip == D_code + lambda R at one block: the block is left out there and one above, coded one below;
    every other output equals the restatement at each of the three."""
    frame, fmt = (32, 16), 0
    geo = R.geometry(32, 16, fmt)
    bits, dq = _bits("huff"), _dequant([28])
    for seed in range(100):
        planes, prev, gold = _content(32, 16, fmt, 300 + seed)
        d = _forced(2, MV, (2, 2))
        src = R.frame_src(planes, 32, 16, fmt, (0, 0, 32, 16))
        w0 = S.stage(geo, src, prev, gold, d["pix"], d["mv"], d["bmv"], dq, bits, lam_fix=0)
        gap = w0["dskip"] - w0["dcode"]
        hit = [k for k in range(geo.nfrags) if gap[k] > 0 and w0["rate"][k] > 0 and gap[k] % w0["rate"][k] == 0]
        if hit:
            break
    assert hit
    k = hit[0]
    lam, fi = int(gap[k] // w0["rate"][k]), int(geo.coded_order[k])
    got = {dl: check(frame, fmt, planes, prev, gold, d, [28], bits, lam=lam + dl) for dl in (-1, 0, 1)}
    assert [int(got[dl]["skf"][fi]) for dl in (-1, 0, 1)] == [0, 1, 1]
    assert int(got[0]["dskip"][k]) == int(got[0]["dcode"][k]) + lam * int(got[0]["rate"][k])


@pytest.mark.parametrize("eight", [False, True], ids=["five", "eight"])
def test_zero_and_non_zero_vectors(hip, eight):
    """The same macro blocks through vector 0 and through a vector: D_skip doubles with the vector; INTRA and MV_FOUR's luma on the way."""
    frame, fmt = (32, 16), 0
    planes, prev, gold = _content(32, 16, fmt, 9)
    base = check(frame, fmt, planes, prev, gold, _forced(2, MV, (0, 0), eight=eight), [30], _bits("huff"))
    moved = check(frame, fmt, planes, prev, gold, _forced(2, MV, (-3, 1), eight=eight), [30], _bits("huff"))
    assert (moved["dskip"] == 2 * base["dskip"]).all() and (base["dskip"] > 0).all()
    intra = check(frame, fmt, planes, prev, gold, _forced(2, INTRA, eight=eight), [30], _bits("huff"))
    assert (intra["dskip"] == base["dskip"]).all()
    if eight:
        four = check(frame, fmt, planes, prev, gold, _forced(2, MV_FOUR, bmv=[[2, 0], [0, 2], [-2, 0], [1, 1]]), [30, 20], _bits("rand"),
                     lam=1 << 30)
        nl = 8
        assert (four["cmap"][:nl] == 2).all() and not four["skf"][:nl].any() and four["skf"][nl:].all()
        check(frame, fmt, planes, prev, gold, _forced(2, GOLDEN_MV, (2, -2)), [30], _bits("huff"))


@pytest.mark.parametrize("fmt", [0, 3], ids=["420", "444"])
def test_prev_equal_to_the_source_leaves_everything_out(hip, fmt):
    """PREV is the source: D_skip = 0, every block the rules would code is left out, the macro blocks lose their mode and their chroma,
    coded as NOMV with an all-zero residual, is uncoded by the rule before the test."""
    frame = (48, 48)
    planes, _, gold = _content(48, 48, fmt, 21)
    prev = [np.flipud(a).copy() for a in planes]
    nmbs = 9
    for d in (_forced(nmbs, MV, (2, 2)), _forced(nmbs, INTRA), _forced(nmbs, MV, (1, -3), eight=False)):
        want = check(frame, fmt, planes, prev, gold, d, [30, 24], _bits("huff"))
        assert not want["cmap"].any() and want["skf"][:36].all() and not want["skf"][36:].any() and want["demoted"].all()
    want = check(frame, fmt, planes, prev, gold, _forced(nmbs, NOMV), [30], _bits("huff"))
    assert not want["cmap"].any() and not want["skf"].any()


def test_prev_far_from_the_source_leaves_nothing_out(hip):
    frame, fmt = (48, 48), 0
    planes, _, gold = _content(48, 48, fmt, 22)
    prev = [np.flipud(255 - a).copy() for a in planes]
    for eight in (False, True):
        d = _decide(frame, fmt, planes, prev, gold, 30, eight)
        want = check(frame, fmt, planes, prev, gold, d, [30, 22, 38], _bits("huff"), ref_pad=5)
        assert not want["skf"].any() and (want["cmap"] != 0).all()
