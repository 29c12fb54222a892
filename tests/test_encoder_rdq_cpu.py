"""th_encode_*'s level choice without a GPU: the controls (TH_ENCCTL_THIP_SET_RD_QUANT, TH_ENCCTL_THIP_GET_RD_QUANT_STATS) and
thip_enc_rdq_stage's refusals on the host library; the restated programme (tests/enc_rdq_ref.py) against a brute force over all 2^n
choices in lexicographic order; the kernel's own programme on the host under sanitizers; the restatement's packets through the
reference decoder; the condition that keeps the GPU packet test from being vacuous; and what the rule buys: bytes at matched SSIM
and PSNR.  Nothing here reaches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import enc_bqi_ref as B
from tests import enc_ref
from tests import enc_rdq_ref as Q
from tests import enc_skip_ref as S
from tests import picture_compare_ref as PC
from tests import refcmp
from tests.test_encoder_bqi_cpu import _ctl, _enc
from tests.test_encoder_mask_cpu import (QUALITIES, SHIFTS, H, W, _bytes_at_matched, _composite, _pan, _psnr, _shifted, _ssim,  # noqa: F401
                                         setup176)

TH_EINVAL, TH_EIMPL = -10, -23
OFF = dict(measured=0, zeroed=[0] * 3, lowered=[0] * 3, emptied=0, rate_before=0, rate_after=0, dist_before=0, dist_after=0, lam=0)


# ---- the controls, on the host library ---------------------------------------------------------------------------------------------
def test_rd_quant_controls():
    """0 and 1..64 accepted, anything else TH_EINVAL; neither call touches the GPU (this machine may have none).  (That the request is
    refused after the first frame needs a frame: tests/test_gpu_encoder_rdq.py.)"""
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_SET_RD_QUANT, E.TH_ENCCTL_THIP_GET_RD_QUANT_STATS) == (0x7222, 0x7223)
    assert C.sizeof(E.RdQuantStats) == 88
    L, enc = _enc()
    try:
        s = E.RdQuantStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_QUANT_STATS, C.byref(s), C.sizeof(s)) == 0   # before any packet
        assert (s.weight, s.measured, list(s.zeroed), list(s.lowered), s.emptied, s.rate_before, s.rate_after, s.dist_before,
                s.dist_after, s.lam, s.rdq_ms) == (0, 0, [0] * 3, [0] * 3, 0, 0, 0, 0, 0, 0, 0.0)
        for v in (0, 1, 64, 0, 5):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_QUANT, v) == (0, v)
        for v in (65, -1, 1 << 20, -(1 << 31)):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_QUANT, v)[0] == TH_EINVAL, v
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_RD_QUANT, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_QUANT, 1, C.c_int64)[0] == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_QUANT, 1, C.c_int16)[0] == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_QUANT_STATS, C.byref(s), C.sizeof(s)) == 0
        assert (s.weight, s.measured) == (5, 0)    # the refused calls changed nothing
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_QUANT_STATS, C.byref(s), C.sizeof(s) - 8) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_QUANT_STATS, None, C.sizeof(s)) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_QUANT, 3) == (0, 3)
        for free in (0x7216, 0x7217, 0x721A, 0x7220, 0x7221, 0x7224):
            assert _ctl(L, enc, free, 0)[0] == TH_EIMPL, hex(free)   # the numbers left free stay free
    finally:
        L.th_encode_free(enc)


def test_python_encoder_rd_quant():
    from theora_amd import encoder as E
    e = E.Encoder(64, 48, 0, 20, inter=True, rd_quant=7)
    assert e.rd_quant == 7 and e.rd_quant_stats() == dict(OFF, weight=7, rdq_ms=0.0)
    e.set_rd_quant(0)
    assert e.rd_quant == 0 and e.rd_quant_stats()["weight"] == 0
    assert e.header_packets() == E.Encoder(64, 48, 0, 20).header_packets()
    with pytest.raises(ValueError):
        e.set_rd_quant(65)
    e.close()
    e = E.Encoder(64, 48, 0, 20, rd_quant=True)   # the recommended weight; accepted with inter frames off
    assert e.rd_quant == E.RD_QUANT_DEFAULT == RECOMMENDED and e.rd_quant_stats()["weight"] == RECOMMENDED
    e.close()
    e = E.Encoder(64, 48, 0, 20)
    assert e.rd_quant == 0 and e.rd_quant_stats()["weight"] == 0
    e.close()


def test_rdq_stage_refusals():
    """Every refusal of thip_enc_rdq_stage comes before a device is touched: the device pointers are never followed."""
    from theora_amd import _lib
    from theora_amd import encoder as E
    EFAULT, EINVAL = _lib.EFAULT, _lib.EINVAL
    L = _lib.load()
    assert L.thip_enc_rdq_stage(None) == EFAULT
    assert C.sizeof(_lib.EncRdqReq) == 248
    dq, bits = np.full((2, 2, 3, 64), 20, np.uint16), np.full((2, 4, 32), 3, np.uint8)
    good = dict(frame=(80, 64), pixel_fmt=0, classes=3, nqis=2, weight=5, pic=(5, 3, 67, 49), lam=100, src=[0x1000, 0x2000, 0x3000],
                src_pitch=[67, 34, 34], prev=[0x4000, 0x5000, 0x6000], gold=[0x7000, 0x8000, 0x9000], ref_pitch=[80, 40, 40], words=0xA000,
                dequant=dq, bits=bits, iscale=0xB000, levels=0xC000, qii=0xD001, cmap=0xE001, jbefore=0x11000, jafter=0x12000,
                rate=0x13000)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return E.rdq_stage(a.pop("frame"), a.pop("pixel_fmt"), a.pop("classes"), a.pop("nqis"), a.pop("weight"), **a)
    for kw in (dict(src=None), dict(src=[0x1000, None, 0x3000]), dict(prev=None), dict(prev=[0x4000, 0x5000, None]), dict(gold=None),
               dict(gold=[None, 0x8000, 0x9000]), dict(words=None), dict(dequant=None), dict(bits=None), dict(levels=None), dict(cmap=None),
               dict(classes=0, levels=None), dict(classes=0, src=None), dict(classes=0, bits=None)):
        assert call(**kw) == EFAULT, kw
    bad_dq = dq.copy()
    bad_dq[1, 1, 2, 63] = 0
    big_dq = dq.copy()
    big_dq[0, 0, 0, 0] = 32768
    bad_bits = bits.copy()
    bad_bits[1, 3, 31] = 65
    for kw in (dict(classes=1), dict(classes=4), dict(classes=-1), dict(classes=2), dict(nqis=0), dict(nqis=4), dict(nqis=-1),
               dict(weight=-1), dict(weight=65), dict(frame=(0, 64)), dict(frame=(80, 0)), dict(frame=(72, 64)), dict(frame=(80, 60)),
               dict(frame=(1 << 20, 64)), dict(frame=(-16, 64)), dict(frame=(65536, 65536), pic=(0, 0, 16, 16)), dict(pixel_fmt=1),
               dict(pixel_fmt=4), dict(pixel_fmt=-1), dict(pic=(0, 0, 0, 49)), dict(pic=(0, 0, 67, 0)), dict(pic=(-1, 3, 67, 49)),
               dict(pic=(5, -1, 67, 49)), dict(pic=(14, 3, 67, 49)), dict(pic=(5, 16, 67, 49)), dict(pic=(0, 0, 81, 49)),
               dict(src_pitch=[66, 34, 34]), dict(src_pitch=[67, 33, 34]), dict(src_pitch=[67, 34, 0]), dict(ref_pitch=[79, 40, 40]),
               dict(ref_pitch=[80, 39, 40]), dict(ref_pitch=[80, 40, 1 << 31]), dict(lam=-2), dict(lam=(1 << 40) + 1),
               dict(dequant=bad_dq), dict(dequant=big_dq), dict(bits=bad_bits), dict(words=0xA008), dict(levels=0xC008),
               dict(iscale=0xB001), dict(jbefore=0x11004), dict(jafter=0x12004), dict(rate=0x13004),
               dict(classes=0, weight=65), dict(classes=0, src_pitch=[66, 34, 34]), dict(classes=0, levels=0xC002)):
        assert call(**kw) == EINVAL, kw
    # classes 2 refuses gold (above) and takes 4-byte aligned words
    assert call(classes=2, gold=None, words=0xA002) == EINVAL
    # (a good request, NULL optional pointers, classes 0 without references: those calls would reach the device)


# ---- the programme against the rule's words ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup32():
    from theora_amd.encoder import Encoder
    return enc_ref.SetupParams(Encoder(16, 16, 0, 32).header_packets()[2])


def _random_block(rng, n, kind):
    lev = np.zeros(64, np.int64)
    lev[rng.choice(np.arange(1, 64), n, replace=False)] = rng.choice([-3, -2, -1, -1, 1, 1, 1, 2, 4, 7, 9, -13], n)
    if kind == "run17":      # +-1 behind a run of 17, then of 18
        lev[:] = 0
        lev[[1, 19, 38]] = (2, -1, 1)
    elif kind == "last62":
        lev[40:] = 0
        lev[62] = 1
    elif kind == "last63":
        lev[40:] = 0
        lev[63] = -1
    lev[0] = rng.integers(-9, 9)
    s = rng.integers(6, 90, 64)
    c = lev * s + (rng.integers(-60, 61, 64) * s) // 100 * rng.choice([1, 2])
    return c, lev, s


def test_programme_against_brute_force(setup32):
    """2 200 random blocks with at most 12 non-zero levels, under the codec's tables, a flat table (every choice of equal token count
    ties) and lambda 0: the programme's levels and J are the brute force's, the first minimiser in lexicographic order."""
    rng = np.random.default_rng(5)
    tables = [Q.full_bits(B.token_bits(setup32, 5)), Q.full_bits(B.token_bits(setup32, 12)), [[4] * 32 for _ in range(4)]]
    changed = ties = 0
    for it in range(2200):
        n = int(rng.integers(9, 13)) if it % 25 == 0 else int(rng.integers(0, 8))
        c, lev, s = _random_block(rng, n, ("run17", "last62", "last63")[it % 40] if it % 40 < 3 else "")
        fb = tables[it % 3]
        lam = int(rng.choice([0, 1, 9, 80, 700, 6000, 1 << 40]))
        r = Q.choose_block(c, lev, s, fb, lam)
        bl, bj = Q.brute_block(c, lev, s, fb, lam)
        assert r["lev"] == bl and r["jafter"] == bj, (it, lev.tolist(), lam)
        assert r["jbefore"] == Q.dist(c, lev, s) + lam * Q.rate(lev, fb) and r["jafter"] <= r["jbefore"]
        assert r["jafter"] == Q.dist(c, r["lev"], s) + lam * r["rate"] and r["rate"] == Q.rate(r["lev"], fb)
        assert r["lev"][0] == lev[0] and all(v == 0 for v, o in zip(r["lev"], lev) if o == 0)
        assert all(v != 0 for v, o in zip(r["lev"], lev) if abs(o) >= 2)
        assert Q.rate(lev, fb) == B.ac_bits(lev, [[b - e for b, e in zip(row, Q.EXTRA_BITS)] for row in fb])
        if lam == 0:
            assert r["lev"] == lev.tolist() and r["zeroed"] == r["lowered"] == 0
        changed += r["lev"] != lev.tolist()
        ties += it % 3 == 2 and lam > 0 and r["jafter"] == r["jbefore"] and n > 0
    assert changed > 500 and ties > 20


def test_a_tie_keeps_the_earlier_coefficient():
    """Two +-1 either of which may go for the same J: the later one goes."""
    fb = [[4] * 32 for _ in range(4)]
    lev = np.zeros(64, np.int64)
    lev[[1, 2, 3]] = (5, 1, 1)
    s = np.full(64, 10)
    c = lev * s
    c[2] = c[3] = 6     # dropping either adds 36 - 16 = 20 and saves one token of 4 bits; dropping both saves two
    r = Q.choose_block(c, lev, s, fb, 5)    # 20 = 5 * 4: every choice ties
    assert r["lev"][:4] == [0, 5, 1, 1] and r["jafter"] == r["jbefore"]
    r = Q.choose_block(c, lev, s, fb, 6)
    assert r["lev"][:4] == [0, 5, 0, 0]
    assert Q.brute_block(c, lev, s, fb, 5)[0][:4] == [0, 5, 1, 1]


def test_programme_on_the_host_under_sanitizers(tmp_path):
    """rdq_walk, the kernel's own programme with the indexing of its LDS arrays, as a stand-alone program under AddressSanitizer and
    UBSan (tests/native/rdq_walk_host.cpp): 4 500 blocks in a wave's layout with everything but the block at work poisoned, against a
    brute force where there are at most 12 non-zero levels, the all +-1 block among the rest."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rdq_walk_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused",
           "-I" + os.path.join(root, "theora_amd", "csrc"), os.path.join(root, "tests", "native", "rdq_walk_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("4500 cases") and r.stdout.rstrip().endswith(" 0 failures"), (r.stdout[-500:], r.stderr[-3000:])


# ---- the packets -------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(case):
    """(headers, packets, reconstructions, frame dicts) of a packet case, coded once."""
    if case not in _CASES:
        from theora_amd.encoder import Encoder
        headers = Encoder(case[1], case[2], case[3], case[4]).header_packets()
        e = Q.case_encoder(case, enc_ref.SetupParams(headers[2]))
        outs, recs = [], []
        for fr in Q.case_frames(case):
            outs.append(e.frame(fr, case[4]))
            recs.append([a.copy() for a in e.recon])
        e.close()
        _CASES[case] = (headers, [o["packet"] for o in outs], recs, outs)
    return _CASES[case]


@pytest.mark.parametrize("case", Q.PACKET_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_reference_decoder_reaches_the_restatements_pictures(case):
    from oracle import ref
    refcmp.need_ref()
    headers, packets, recs, _ = _case(case)
    rd = ref.RefDecoder(headers)
    try:
        for n, (pkt, rec) in enumerate(zip(packets, recs)):
            assert rd.packetin(pkt)[0] == 0, n
            pic = rd.ycbcr_out()
            for p in range(3):
                assert np.array_equal(np.asarray(pic[p]), rec[p]), (n, p)
    finally:
        rd.close()


@pytest.mark.parametrize("case", Q.PACKET_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_packet_cases_are_not_vacuous(case):
    """w = 0 is SkipEncoder's stream byte for byte; w > 0 changes every packet, and at quality 32 at least 5 % of the coded blocks of
    every frame; the statistics say what happened."""
    headers, packets, _, outs = _case(case)
    kind, fw, fh, fmt, q, nf, kf, modes, delta, k, rd, skip, w = case
    setup = enc_ref.SetupParams(headers[2])
    off = Q.case_encoder(case, setup, w=0)
    base = S.SkipEncoder(fw, fh, fmt, (0, 0, fw, fh), setup, kf, 6, delta, k, modes, rd, skip)
    for n, fr in enumerate(Q.case_frames(case)):
        a, b = off.frame(fr, q), base.frame(fr, q)
        assert a["packet"] == b["packet"] and a["rdq"] == dict(OFF, weight=0), n
        o = outs[n]
        assert o["packet"] != a["packet"] and o["key"] == a["key"], n
        st = o["rdq"]
        assert st["weight"] == w and st["measured"] == 1 and sum(st["zeroed"]) > 0
        assert st["rate_after"] < st["rate_before"] and st["dist_after"] > st["dist_before"] and st["lam"] > 0
        if q == 32:
            assert o["rdq_changed"] * 20 >= sum(o["coded"]), (n, o["rdq_changed"], o["coded"])
    off.close()
    base.close()
    assert any(o["key"] for o in outs) and (kf == 1 or any(not o["key"] for o in outs))
    assert sum(sum(o["rdq"]["lowered"]) for o in outs) > 0


# ---- what it buys ------------------------------------------------------------------------------------------------------------------
RECOMMENDED = 3
_SWEEPS = {}


def _clip(name):
    if name == "static":
        return S.clip("static", W, H, 0, 3, seed=2)
    first = _composite() if name == "composite" else _pan()
    return [first] + [_shifted(first, *s) for s in SHIFTS]


def _sweep(setup, name, skip, w):
    """Per quality and frame: (bytes, mean Y window_q20, Y sse) of the key frame and the two inter frames of clip `name`, eight modes."""
    if (name, skip, w) not in _SWEEPS:
        rows = []
        for q in QUALITIES:
            e = Q.RdqEncoder(W, H, 0, (0, 0, W, H), setup, 64, 6, modes=True, skip=skip, w=w)
            fr_rows = []
            for fr in _clip(name):
                r = e.frame(fr, q)
                rec = np.asarray(e.recon[0], np.int64)
                fr_rows.append((len(r["packet"]), float(PC.window_q20(fr[0], rec).mean()), int(((np.asarray(fr[0], np.int64) - rec) ** 2).sum())))
            e.close()
            rows.append(fr_rows)
        _SWEEPS[(name, skip, w)] = rows
    return _SWEEPS[(name, skip, w)]


def _over(rows, frames):
    return [(sum(r[f][0] for f in frames), float(np.mean([r[f][1] for f in frames])), sum(r[f][2] for f in frames)) for r in rows]


# (clip, skip decision, frames) -> the bytes at matched mean Y SSIM and at matched Y PSNR, w = RECOMMENDED against w = 0, as measured
# (DESIGN.md section 5.19 has the table, with the other weights).  Where a gain was measured the test asserts half of it (the midpoint
# between the figure and 1); where none was, it pins the figure within 0.005.
MEASURED = {("pan", False, "inter"): (0.9121, 0.8694), ("pan", True, "inter"): (0.9615, 0.9031),
            ("composite", False, "inter"): (0.8675, 0.8328), ("composite", True, "inter"): (0.8667, 0.8394),
            ("static", False, "inter"): (0.8665, 0.7828), ("static", True, "inter"): (0.9182, 0.8436),
            ("pan", False, "key"): (0.9862, 0.9276), ("composite", False, "key"): (0.9987, 0.9685), ("static", False, "key"): (1.0171, 0.9273)}


@pytest.mark.parametrize("name,skip,what", list(MEASURED), ids=lambda v: str(v))
def test_what_the_rule_buys(setup176, name, skip, what):
    frames = (1, 2) if what == "inter" else (0,)
    off, on = _over(_sweep(setup176, name, skip, 0), frames), _over(_sweep(setup176, name, skip, RECOMMENDED), frames)
    got = (_bytes_at_matched(off, on, _ssim), _bytes_at_matched(off, on, _psnr))
    print("\n%s, skip %s, %s: bytes at matched Y SSIM %.4f, at matched Y PSNR %.4f" % (name, skip, what, got[0], got[1]))
    print("  off", [(r[0], round(r[1]), r[2]) for r in off])
    print("  on ", [(r[0], round(r[1]), r[2]) for r in on])
    for metric, g, m in zip(("SSIM", "PSNR"), got, MEASURED[(name, skip, what)]):
        if m < 0.995:
            assert g <= (1 + m) / 2, (metric, g, m)
        else:
            assert abs(g - m) < 0.005, (metric, g, m)
