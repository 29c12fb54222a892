"""The direct stage entries (thip_enc_{inter,rate,mask,roi,rd,skip,rdq,tok,fq}_stage of include/theora_hip.h) refuse alike: one table
of requests that are wrong in two ways at once, or wrong at an edge, with the code each entry answers.  The codes are the contract of
the entries' shared frame, picture and plane rules (the order of the checks included): they were recorded from the entries as they
stood when each still carried its own copy of those rules.  No GPU: every request here is refused before a device is touched, the
pointers are addresses nobody follows."""
import numpy as np
import pytest

from theora_amd import encoder as E

A = 0x100000    # an address aligned for every field
EFAULT, EINVAL = -1, -10

_DQ1, _DQ2 = np.full(384, 20, np.uint16), np.full(768, 20, np.uint16)
_BITS = np.full(256, 3, np.uint8)
_PLANES = dict(pic=(5, 3, 67, 49), src=[A + 1, A + 2, A + 3], src_pitch=[67, 34, 34])
_REFS = dict(prev=[A] * 3, ref_pitch=[80, 40, 40])
_FRAME = dict(frame=(80, 64), pixel_fmt=0)

# each entry's known-good request (those of the entries' own refusal tests, on one frame), the tables it range-checks as
# name -> (lowest, highest), and the pointers it wants aligned
ENTRIES = {
    "inter": (E.inter_stage, dict(_FRAME, **_PLANES, **_REFS, stages=7, classes=2, lam=5, dequant=_DQ1, gold=None, stats=A, words=A,
                                  words_from_stats=A, levels=A, dcq=A, cmap=A, dcr=A),
              dict(dequant=(1, 32767)), ("stats", "words", "words_from_stats", "levels", "dcq", "dcr")),
    "rate": (E.rate_stage, dict(_FRAME, **_PLANES, **_REFS, inter=1, stages=15, groups=0, fixed=28, steps=np.full(6 * 64 * 64, 8, np.uint16),
                                lam=np.ones(64, np.int32), lens=np.ones(80 * 32, np.uint8), stats=A, coef=A, qdc=A, coded=A, cls=A, partial=A,
                                est=A),
             dict(steps=(1, 32767), lam=(0, 1 << 24)), ("stats", "coef", "qdc", "coded", "cls", "partial", "est")),
    "mask": (E.mask_stage, dict(_FRAME, **_PLANES, ratio=4, act=A, avg=A, iscale=A), {}, ("act", "avg", "iscale")),
    "roi": (E.roi_stage, dict(_FRAME, pic=_PLANES["pic"], map_size=(5, 4), map_pitch=8, map=A + 1, mask_iscale=A, iscale=A, stats=A), {},
            ("mask_iscale", "iscale", "stats")),
    "rd": (E.rd_stage, dict(_FRAME, **_PLANES, **_REFS, gold=[A] * 3, stages=3, lambda_search=30, lambda_rd=100, dequant=_DQ1,
                            bits=np.full(320, 3, np.uint8), cand=A, costs=A, words=A),
           dict(dequant=(1, 32767)), ("cand", "costs", "words")),
    "skip": (E.skip_stage, dict(_FRAME, **_PLANES, **_REFS, gold=[A] * 3, classes=3, nqis=2, lam=100, words=A, dequant=_DQ2, bits=_BITS,
                                iscale=A, levels=A, dcq=A, qii=A + 1, cmap=A + 1, skf=A + 1, dcode=A, rate=A, dskip=A),
             dict(dequant=(1, 32767), bits=(0, 64)), ("words", "levels", "dcq", "iscale", "dcode", "rate", "dskip")),
    "rdq": (E.rdq_stage, dict(_FRAME, **_PLANES, **_REFS, gold=[A] * 3, classes=3, nqis=2, weight=5, lam=100, words=A, dequant=_DQ2,
                              bits=_BITS, iscale=A, levels=A, qii=A + 1, cmap=A + 1, jbefore=A, jafter=A, rate=A),
            dict(dequant=(1, 32767), bits=(0, 64)), ("words", "levels", "iscale", "jbefore", "jafter", "rate")),
    "tok": (E.tok_stage, dict(_FRAME, classes=0, stages=7, levels=A, dcq=A, dcr=A, cmap=A + 1, tok=A, mask=A, chunk_cnt=A, chunk_base=A,
                              list_len=A, overflow=A, out=A, out_cap=1 << 20),
            {}, ("levels", "dcq", "dcr", "mask", "tok", "chunk_cnt", "chunk_base", "list_len", "overflow", "out")),
    "fq": (E.fq_stage, dict(_FRAME, **_PLANES, **_REFS, gold=[A] * 3, classes=3, nqis=2, words=A, dequant=_DQ2, bits=_BITS, iscale=A,
                            levels=A, dcq=A, qii=A + 1, cmap=A + 1, dcr=A, overflow=A),
           dict(dequant=(1, 32767), bits=(0, 64)), ("words", "levels", "dcq", "dcr", "iscale", "overflow")),
}

# one macro block row over every entry's cap of 1 << 24 blocks: 4:2:0 at 16384 pixels a row has 6144 blocks a macro block row, and
# 2730 such rows lie under the cap
_OVER = (16384, 16 * 2731)
assert 6144 * 2730 <= 1 << 24 < 6144 * 2731
_BAD_PIC = (14, 3, 67, 49)      # 14 + 67 > 80
_ONE_NULL = [A + 1, None, A + 3]


def _cases():
    out = []
    for name, (fn, good, tables, aligned) in ENTRIES.items():
        def add(what, **change):
            out.append(("%s: %s" % (name, what), fn, dict(good, **change)))
        if "src" in good:
            add("(a) a bad rectangle and a NULL src plane", pic=_BAD_PIC, src=_ONE_NULL)
            add("(b) a NULL src plane and a small src_pitch", src=_ONE_NULL, src_pitch=[66, 34, 34])
        if name == "mask":   # (the one entry with a check of its own between the planes and their pitches)
            add("(b) a NULL output and a small src_pitch", act=None, src_pitch=[66, 34, 34])
        if "gold" in good and "classes" in good:
            add("(c) gold with classes 2 and a small ref_pitch", classes=2, gold=[A] * 3, ref_pitch=[79, 40, 40])
            add("(d) classes 3 with one gold plane missing", classes=3, gold=[A, None, A])
        add("(e) one macro block row over the cap", frame=_OVER, **(dict(ref_pitch=[16384, 8192, 8192]) if "ref_pitch" in good else {}))
        for tab, (lo, hi) in tables.items():
            for at in (0, -1):
                for v in ([lo - 1] if lo > 0 or tab == "lam" else []) + [hi + 1]:
                    t = good[tab].astype(np.int64)
                    t[at] = v
                    add("(f) %s[%s] = %d" % (tab, "last" if at else "0", v), **{tab: t})
        for ptr in aligned:
            add("(g) %s off by a byte" % ptr, **{ptr: A + 1})
    return out


CASES = _cases()

# what the entries answered before their rules were stated once
EXPECTED = {
    'inter: (a) a bad rectangle and a NULL src plane': EINVAL,
    'inter: (b) a NULL src plane and a small src_pitch': EFAULT,
    'inter: (c) gold with classes 2 and a small ref_pitch': EINVAL,
    'inter: (d) classes 3 with one gold plane missing': EFAULT,
    'inter: (e) one macro block row over the cap': EINVAL,
    'inter: (f) dequant[0] = 0': EINVAL,
    'inter: (f) dequant[0] = 32768': EINVAL,
    'inter: (f) dequant[last] = 0': EINVAL,
    'inter: (f) dequant[last] = 32768': EINVAL,
    'inter: (g) stats off by a byte': EINVAL,
    'inter: (g) words off by a byte': EINVAL,
    'inter: (g) words_from_stats off by a byte': EINVAL,
    'inter: (g) levels off by a byte': EINVAL,
    'inter: (g) dcq off by a byte': EINVAL,
    'inter: (g) dcr off by a byte': EINVAL,
    'rate: (a) a bad rectangle and a NULL src plane': EINVAL,
    'rate: (b) a NULL src plane and a small src_pitch': EFAULT,
    'rate: (e) one macro block row over the cap': EINVAL,
    'rate: (f) steps[0] = 0': EINVAL,
    'rate: (f) steps[0] = 32768': EINVAL,
    'rate: (f) steps[last] = 0': EINVAL,
    'rate: (f) steps[last] = 32768': EINVAL,
    'rate: (f) lam[0] = -1': EINVAL,
    'rate: (f) lam[0] = 16777217': EINVAL,
    'rate: (f) lam[last] = -1': EINVAL,
    'rate: (f) lam[last] = 16777217': EINVAL,
    'rate: (g) stats off by a byte': EINVAL,
    'rate: (g) coef off by a byte': EINVAL,
    'rate: (g) qdc off by a byte': EINVAL,
    'rate: (g) coded off by a byte': EINVAL,
    'rate: (g) cls off by a byte': EINVAL,
    'rate: (g) partial off by a byte': EINVAL,
    'rate: (g) est off by a byte': EINVAL,
    'mask: (a) a bad rectangle and a NULL src plane': EINVAL,
    'mask: (b) a NULL src plane and a small src_pitch': EFAULT,
    'mask: (b) a NULL output and a small src_pitch': EFAULT,
    'mask: (e) one macro block row over the cap': EINVAL,
    'mask: (g) act off by a byte': EINVAL,
    'mask: (g) avg off by a byte': EINVAL,
    'mask: (g) iscale off by a byte': EINVAL,
    'roi: (e) one macro block row over the cap': EINVAL,
    'roi: (g) mask_iscale off by a byte': EINVAL,
    'roi: (g) iscale off by a byte': EINVAL,
    'roi: (g) stats off by a byte': EINVAL,
    'rd: (a) a bad rectangle and a NULL src plane': EINVAL,
    'rd: (b) a NULL src plane and a small src_pitch': EFAULT,
    'rd: (e) one macro block row over the cap': EINVAL,
    'rd: (f) dequant[0] = 0': EINVAL,
    'rd: (f) dequant[0] = 32768': EINVAL,
    'rd: (f) dequant[last] = 0': EINVAL,
    'rd: (f) dequant[last] = 32768': EINVAL,
    'rd: (g) cand off by a byte': EINVAL,
    'rd: (g) costs off by a byte': EINVAL,
    'rd: (g) words off by a byte': EINVAL,
    'skip: (a) a bad rectangle and a NULL src plane': EINVAL,
    'skip: (b) a NULL src plane and a small src_pitch': EFAULT,
    'skip: (c) gold with classes 2 and a small ref_pitch': EINVAL,
    'skip: (d) classes 3 with one gold plane missing': EFAULT,
    'skip: (e) one macro block row over the cap': EINVAL,
    'skip: (f) dequant[0] = 0': EINVAL,
    'skip: (f) dequant[0] = 32768': EINVAL,
    'skip: (f) dequant[last] = 0': EINVAL,
    'skip: (f) dequant[last] = 32768': EINVAL,
    'skip: (f) bits[0] = 65': EINVAL,
    'skip: (f) bits[last] = 65': EINVAL,
    'skip: (g) words off by a byte': EINVAL,
    'skip: (g) levels off by a byte': EINVAL,
    'skip: (g) dcq off by a byte': EINVAL,
    'skip: (g) iscale off by a byte': EINVAL,
    'skip: (g) dcode off by a byte': EINVAL,
    'skip: (g) rate off by a byte': EINVAL,
    'skip: (g) dskip off by a byte': EINVAL,
    'rdq: (a) a bad rectangle and a NULL src plane': EINVAL,
    'rdq: (b) a NULL src plane and a small src_pitch': EFAULT,
    'rdq: (c) gold with classes 2 and a small ref_pitch': EINVAL,
    'rdq: (d) classes 3 with one gold plane missing': EFAULT,
    'rdq: (e) one macro block row over the cap': EINVAL,
    'rdq: (f) dequant[0] = 0': EINVAL,
    'rdq: (f) dequant[0] = 32768': EINVAL,
    'rdq: (f) dequant[last] = 0': EINVAL,
    'rdq: (f) dequant[last] = 32768': EINVAL,
    'rdq: (f) bits[0] = 65': EINVAL,
    'rdq: (f) bits[last] = 65': EINVAL,
    'rdq: (g) words off by a byte': EINVAL,
    'rdq: (g) levels off by a byte': EINVAL,
    'rdq: (g) iscale off by a byte': EINVAL,
    'rdq: (g) jbefore off by a byte': EINVAL,
    'rdq: (g) jafter off by a byte': EINVAL,
    'rdq: (g) rate off by a byte': EINVAL,
    'tok: (e) one macro block row over the cap': EINVAL,
    'tok: (g) levels off by a byte': EINVAL,
    'tok: (g) dcq off by a byte': EINVAL,
    'tok: (g) dcr off by a byte': EINVAL,
    'tok: (g) mask off by a byte': EINVAL,
    'tok: (g) tok off by a byte': EINVAL,
    'tok: (g) chunk_cnt off by a byte': EINVAL,
    'tok: (g) chunk_base off by a byte': EINVAL,
    'tok: (g) list_len off by a byte': EINVAL,
    'tok: (g) overflow off by a byte': EINVAL,
    'tok: (g) out off by a byte': EINVAL,
    'fq: (a) a bad rectangle and a NULL src plane': EINVAL,
    'fq: (b) a NULL src plane and a small src_pitch': EFAULT,
    'fq: (c) gold with classes 2 and a small ref_pitch': EINVAL,
    'fq: (d) classes 3 with one gold plane missing': EFAULT,
    'fq: (e) one macro block row over the cap': EINVAL,
    'fq: (f) dequant[0] = 0': EINVAL,
    'fq: (f) dequant[0] = 32768': EINVAL,
    'fq: (f) dequant[last] = 0': EINVAL,
    'fq: (f) dequant[last] = 32768': EINVAL,
    'fq: (f) bits[0] = 65': EINVAL,
    'fq: (f) bits[last] = 65': EINVAL,
    'fq: (g) words off by a byte': EINVAL,
    'fq: (g) levels off by a byte': EINVAL,
    'fq: (g) dcq off by a byte': EINVAL,
    'fq: (g) dcr off by a byte': EINVAL,
    'fq: (g) iscale off by a byte': EINVAL,
    'fq: (g) overflow off by a byte': EINVAL,
}


def test_the_table_is_whole():
    assert [c[0] for c in CASES] == list(EXPECTED)
    assert {c[0].split(":")[0] for c in CASES} == set(ENTRIES) and len(ENTRIES) == 9


@pytest.mark.parametrize("what,fn,kw", CASES, ids=[c[0] for c in CASES])
def test_refusal(what, fn, kw, capfd):
    assert fn(**kw) == EXPECTED[what]
    assert "theora_hip" not in capfd.readouterr().err   # (refused by the rules, not by a device that is not there)

