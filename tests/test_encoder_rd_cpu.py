"""th_encode_*'s rate-distortion mode decision without a GPU: the controls (TH_ENCCTL_THIP_SET_RD_MODES, TH_ENCCTL_THIP_GET_RD_STATS)
and thip_enc_rd_stage's refusals on the host library; the restatement of the rule (tests/enc_rd_ref.py) against a scalar loop over
tests/enc_ref.block_tokens, at its exceptions (an all-zero NOMV block, the tie of GOLDEN_NOMV while GOLD is PREV, the INTRA DC
charge) and against the decoders of its own packets; the condition that keeps the GPU packet test from being vacuous; and what the
rule buys: bytes at matched SSIM against the SAD cascade.  Nothing here reaches a device."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import enc_modes_ref as M
from tests import enc_rd_ref as RD
from tests import enc_ref
from tests import inter_stage_ref as SR
from tests.enc_inter_ref import predict
from tests.enc_ref import ZIGZAG
from tests.test_encoder_bqi_cpu import _ctl, _decode_check, _enc, trace_env   # noqa: F401  (trace_env: a fixture)
from tests.test_encoder_mask_cpu import (QUALITIES, SHIFTS, H, W, _bytes_at_matched, _composite, _pan, _psnr, _shifted, _ssim, setup64,  # noqa: F401
                                         setup176)

TH_EINVAL, TH_EIMPL = -10, -23


# ---- the controls, on the host library ---------------------------------------------------------------------------------------------
def test_rd_controls():
    """0 and 1 accepted, anything else TH_EINVAL; neither call touches the GPU (this machine may have none)."""
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_SET_RD_MODES, E.TH_ENCCTL_THIP_GET_RD_STATS) == (0x7218, 0x7219)
    assert C.sizeof(E.RdStats) == 40
    L, enc = _enc()
    try:
        s = E.RdStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_STATS, C.byref(s), C.sizeof(s)) == 0   # before any packet
        assert (s.on, s.measured, list(s.huff), s.lam, s.rd_ms) == (0, 0, [0] * 4, 0, 0.0)
        for v in (0, 1, 0, 1):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_MODES, v) == (0, v)   # accepted with inter frames and eight modes off
        for v in (-1, 2, 3, 64, 1 << 20, -(1 << 31)):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_MODES, v)[0] == TH_EINVAL, v
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_RD_MODES, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_MODES, 1, C.c_int64)[0] == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_STATS, C.byref(s), C.sizeof(s)) == 0
        assert (s.on, s.measured) == (1, 0)
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_STATS, C.byref(s), C.sizeof(s) - 8) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_RD_STATS, None, C.sizeof(s)) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_MODES, 1)[0] == 0
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_RD_MODES, 1) == (0, 1)
        for free in (0x7216, 0x7217, 0x721A):
            assert _ctl(L, enc, free, 0)[0] == TH_EIMPL, hex(free)   # the numbers left free stay free
    finally:
        L.th_encode_free(enc)


def test_python_encoder_rd():
    from theora_amd.encoder import Encoder
    e = Encoder(64, 48, 0, 20, inter=True, all_modes=True, rd_modes=True)
    assert e.rd_modes and e.rd_stats() == dict(on=1, measured=0, huff=[0] * 4, lam=0, rd_ms=0.0)
    e.set_rd_modes(False)
    assert not e.rd_modes and e.rd_stats()["on"] == 0
    assert e.header_packets() == Encoder(64, 48, 0, 20).header_packets()
    e.close()
    e = Encoder(64, 48, 0, 20)
    assert not e.rd_modes and e.rd_stats()["on"] == 0
    e.close()


def test_rd_stage_refusals():
    """Every refusal of thip_enc_rd_stage comes before a device is touched: the device pointers are never followed."""
    from theora_amd import _lib
    from theora_amd import encoder as E
    EFAULT, EINVAL = _lib.EFAULT, _lib.EINVAL
    L = _lib.load()
    assert L.thip_enc_rd_stage(None) == EFAULT
    assert C.sizeof(_lib.EncRdReq) == 200 and C.sizeof(_lib.EncInterReq) == 224
    assert (_lib.ENC_RD_CAND, _lib.ENC_RD_DECIDE) == (1, 2)
    dq, bits = np.full((2, 3, 64), 20, np.uint16), np.full((2, 5, 32), 3, np.uint8)
    good = dict(frame=(80, 64), pixel_fmt=0, stages=3, pic=(5, 3, 67, 49), lambda_search=30, lambda_rd=100, src=[0x1000, 0x2000, 0x3000],
                src_pitch=[67, 34, 34], prev=[0x4000, 0x5000, 0x6000], gold=[0x7000, 0x8000, 0x9000], ref_pitch=[80, 40, 40], dequant=dq,
                bits=bits, cand=0xA000, costs=0xB000, words=0xC000)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return E.rd_stage(a.pop("frame"), a.pop("pixel_fmt"), a.pop("stages"), **a)
    for kw in (dict(src=None), dict(src=[0x1000, None, 0x3000]), dict(prev=None), dict(prev=[0x4000, 0x5000, None]), dict(gold=None),
               dict(gold=[None, 0x8000, 0x9000]), dict(cand=None), dict(words=None), dict(dequant=None), dict(bits=None),
               dict(stages=1, cand=None), dict(stages=2, cand=None), dict(stages=2, words=None)):
        assert call(**kw) == EFAULT, kw
    bad_dq = dq.copy()
    bad_dq[1, 2, 63] = 0
    big_dq = dq.copy()
    big_dq[0, 0, 0] = 32768
    for kw in (dict(stages=0), dict(stages=4), dict(stages=-1), dict(frame=(0, 64)), dict(frame=(80, 0)), dict(frame=(72, 64)),
               dict(frame=(80, 60)), dict(frame=(1 << 20, 64)), dict(frame=(-16, 64)), dict(frame=(65536, 65536), pic=(0, 0, 16, 16)),
               dict(pixel_fmt=1), dict(pixel_fmt=4), dict(pixel_fmt=-1), dict(pic=(0, 0, 0, 49)), dict(pic=(0, 0, 67, 0)),
               dict(pic=(-1, 3, 67, 49)), dict(pic=(5, -1, 67, 49)), dict(pic=(14, 3, 67, 49)), dict(pic=(5, 16, 67, 49)),
               dict(pic=(0, 0, 81, 49)), dict(src_pitch=[66, 34, 34]), dict(src_pitch=[67, 33, 34]), dict(src_pitch=[67, 34, 0]),
               dict(ref_pitch=[79, 40, 40]), dict(ref_pitch=[80, 39, 40]), dict(ref_pitch=[80, 40, 1 << 31]), dict(lambda_search=-1),
               dict(lambda_search=(1 << 24) + 1), dict(lambda_rd=-1), dict(lambda_rd=(1 << 24) + 1), dict(dequant=bad_dq),
               dict(dequant=big_dq), dict(cand=0xA008), dict(words=0xC004), dict(costs=0xB004)):
        assert call(**kw) == EINVAL, kw
    # (costs may be NULL, and a search alone needs neither table nor words: those calls would reach the device)


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def _setup(q=32):
    from theora_amd.encoder import Encoder
    return enc_ref.SetupParams(Encoder(16, 16, 0, q).header_packets()[2])


def _tabs(setup, qi):
    return {(t, p): setup.qmat(t, p, qi)[ZIGZAG] for t in range(2) for p in range(3)}


def _one_mb(fmt, seed, kind="natural"):
    """(geo, src, prev, gold): one macro block of content (bitstream rows), the references other crops of the same image."""
    geo = SR.geometry(16, 16, fmt)
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    out = []
    for k, (ox, oy) in enumerate(((8, 8), (9, 8), (6, 10))):
        pl = []
        for p in range(3):
            sx, sy = (hd, vd) if p else (0, 0)
            big = enc_ref.content(kind, (48, 48), seed + p).astype(np.int64)
            if k == 0 and kind == "natural":
                big = np.clip(big + enc_ref.content("noise", (48, 48), seed + 9 + p).astype(np.int64) // 16 - 8, 0, 255)
            pl.append(np.ascontiguousarray(big[oy:oy + (16 >> sy), ox:ox + (16 >> sx)]))
        out.append(pl)
    src, prev, gold = out
    return geo, src, [a.astype(np.uint8) for a in prev], [a.astype(np.uint8) for a in gold]


def _scalar_costs(geo, src, prev, gold, ms, tabs, setup, hti, lam, charge_dc=True):
    """J [6] of the one macro block by the rule's words, a block at a time over enc_ref.block_tokens."""
    J = []
    for m, pix in enumerate(RD.CANDS):
        pixv, mv, bmv = RD.candidate(ms, m)
        fvx, fvy = M.fragment_vectors(geo, pixv, mv, bmv)
        total, dc0 = 0, None
        for fi in range(geo.nfrags):
            p = int(geo.plane_of[fi])
            g = geo.planes[p]
            loc = fi - g["froffset"]
            fy, fx = loc // g["nhfrags"], loc % g["nhfrags"]
            Y, X = np.mgrid[fy * 8:fy * 8 + 8, fx * 8:fx * 8 + 8]
            if pix == M.INTRA:
                pred = 128
            else:
                ref = gold if pix in (M.GOLDEN_NOMV, M.GOLDEN_MV) else prev
                pred = predict(ref[p], X, Y, int(fvx[fi]), int(fvy[fi]), p > 0 and geo.hdec, p > 0 and geo.vdec)
            c = oracle.fdct8x8_batch((src[p][Y, X] - pred).reshape(1, 64).astype(np.int16))
            s = np.asarray(tabs[(0 if pix == M.INTRA else 1, p)], np.int64)
            l = oracle.quantize_batch(c, s.astype(np.uint16))[0][0].astype(np.int64)
            c = c[0].astype(np.int64)
            if pix == M.NOMV and not l.any():
                total += int((c * c).sum())
                continue
            v = l.copy()
            if pix == M.INTRA and p == 0 and charge_dc:
                if fi == 0:
                    dc0 = int(l[0])
                else:
                    v[0] -= dc0
            bits = 0
            for t in enc_ref.block_tokens(v):
                tab = setup.codes[16 * enc_ref.huff_group(t[0]) + hti[(2 if t[0] else 0) + int(p > 0)]]
                bits += len(tab[0]) if t[1] == "EOB" else len(tab[t[1]]) + t[3]
            total += int(((c - l * s) ** 2).sum()) + lam * bits
        J.append(total + lam * RD.HEADER_BITS[m])
    return J


@pytest.mark.parametrize("fmt", [0, 2, 3], ids=["420", "422", "444"])
def test_costs_against_a_scalar_loop(fmt):
    setup = _setup()
    geo, src, prev, gold = _one_mb(fmt, 3 + fmt)
    assert geo.nfrags == {0: 6, 2: 8, 3: 12}[fmt]
    ms = M.search_all(src[0], prev[0], gold[0])
    hti = [3, 9, 5, 12]
    for qi in (10, 40):
        tabs = _tabs(setup, qi)
        lam = RD.rd_lambda(tabs[(1, 0)][1])
        J = RD.rd_costs(geo, src, prev, gold, ms, tabs, RD.bits_table(setup, hti), lam)
        assert J.shape == (1, 6) and J.dtype == np.int64
        want = _scalar_costs(geo, src, prev, gold, ms, tabs, setup, hti, lam)
        assert J[0].tolist() == want, (qi, J[0].tolist(), want)
        assert len(set(want)) == 6   # (six different costs: nothing is compared with itself)
        d = RD.rd_decide(ms, J)
        assert int(d["cand"][0]) == int(np.argmin(want)) and int(d["pix"][0]) == RD.CANDS[int(np.argmin(want))]


def test_lambda_and_constants():
    setup = _setup()
    for qi in (0, 16, 48, 63):
        s1 = int(setup.qmat(1, 0, qi)[ZIGZAG][1])
        assert RD.rd_lambda(s1) == (s1 * s1 * 40) >> 7
    assert RD.HEADER_BITS == (1, 15, 55, 5, 18, 4)   # a mode code of 1, 3, 7, 5, 6, 4 bits and six bits a component of 0, 1, 4, 0, 1, 0 vectors
    assert RD.CANDS == (M.NOMV, M.MV, M.MV_FOUR, M.GOLDEN_NOMV, M.GOLDEN_MV, M.INTRA)


def test_an_all_zero_nomv_block_is_uncoded():
    """A residual that quantises to nothing: under candidate 0 the macro block costs its header bit and the squared coefficients;
    under GOLDEN_NOMV (GOLD = PREV here) the same distortion and every block's EOB besides."""
    setup = _setup()
    geo, src, prev, gold = _one_mb(0, 11)
    rng = np.random.default_rng(2)
    src = [np.clip(a.astype(np.int64) + rng.integers(-1, 2, a.shape), 0, 255) for a in prev]
    ms = M.search_all(src[0], prev[0], prev[0])
    tabs, hti = _tabs(setup, 0), [5, 5, 5, 5]
    lam = RD.rd_lambda(tabs[(1, 0)][1])
    bits = RD.bits_table(setup, hti)
    cost, D, R, lev, dct = RD.block_costs(geo, src, prev, prev, ms, tabs, bits, lam, 0)
    assert not lev.any() and (dct != 0).any()
    energy = int((dct * dct).sum())
    J = RD.rd_costs(geo, src, prev, prev, ms, tabs, bits, lam)
    assert int(J[0, 0]) == energy + lam * 1
    eob = 4 * int(bits[0, 0, 0]) + 2 * int(bits[1, 0, 0])
    assert int(J[0, 3]) == energy + lam * (eob + 5) and R.tolist() == [int(bits[0, 0, 0])] * 4 + [int(bits[1, 0, 0])] * 2
    assert J[0].tolist() == _scalar_costs(geo, src, prev, prev, ms, tabs, setup, hti, lam)
    assert int(RD.rd_decide(ms, J)["cand"][0]) == 0


@pytest.mark.parametrize("fmt", [0, 3], ids=["420", "444"])
def test_gold_is_prev_costs_four_lambda_more(fmt):
    """While GOLD is PREV candidate 3 predicts what candidate 0 predicts: where every block has a level J_3 = J_0 + 4 lambda exactly
    (H_3 - H_0), and with uncoded blocks more than that; the tie of equal predictions never arises, candidate 3 never wins."""
    setup = _setup()
    geo, src, prev, _ = _one_mb(fmt, 5, kind="noise")
    ms = M.search_all(src[0], prev[0], prev[0])
    for qi in (20, 63):
        tabs = _tabs(setup, qi)
        lam = RD.rd_lambda(tabs[(1, 0)][1])
        bits = RD.bits_table(setup, [5] * 4)
        lev = RD.block_costs(geo, src, prev, prev, ms, tabs, bits, lam, 0)[3]
        assert (lev != 0).any(1).all()   # every block coded
        J = RD.rd_costs(geo, src, prev, prev, ms, tabs, bits, lam)
        assert int(J[0, 3]) == int(J[0, 0]) + 4 * lam
        assert int(J[0, 4]) == int(J[0, 1]) + 3 * lam and ms["gvx"][0] == ms["mvx"][0] and ms["gvy"][0] == ms["mvy"][0]
    # lambda 0: J_3 = J_0, and the lower index takes the tie
    J0 = RD.rd_costs(geo, src, prev, prev, ms, tabs, bits, 0)
    assert int(J0[0, 3]) == int(J0[0, 0])
    J0[:, [1, 2, 4, 5]] = J0[:, [0]] + 1
    assert int(RD.rd_decide(ms, J0)["cand"][0]) == 0


def test_the_intra_dc_charge():
    """INTRA luma blocks 1..3 are charged their quantised DC less luma block 0's; block 0 and chroma their own."""
    setup = _setup()
    geo, src, prev, gold = _one_mb(0, 7)
    ms = M.search_all(src[0], prev[0], gold[0])
    tabs, hti = _tabs(setup, 32), [5, 5, 5, 5]
    lam = RD.rd_lambda(tabs[(1, 0)][1])
    bits = RD.bits_table(setup, hti)
    cost, D, R, lev, dct = RD.block_costs(geo, src, prev, gold, ms, tabs, bits, lam, 5)
    b5 = [np.asarray(bits, np.int64)[c].tolist() for c in range(2)]
    for fi in range(6):
        v = lev[fi].copy()
        if 1 <= fi < 4:
            v[0] -= lev[0, 0]
        assert int(R[fi]) == RD.block_bits(v, b5[int(fi >= 4)]), fi
    plain = sum(RD.block_bits(lev[fi], b5[int(fi >= 4)]) for fi in range(6))
    assert abs(int(lev[0, 0])) > 8 and int(R.sum()) < plain   # a picture's DCs lie together: the charge is the smaller
    J = RD.rd_costs(geo, src, prev, gold, ms, tabs, bits, lam)
    assert int(J[0, 5]) == int(D.sum()) + lam * (int(R.sum()) + 4)
    assert J[0].tolist() != _scalar_costs(geo, src, prev, gold, ms, tabs, setup, hti, lam, charge_dc=False)


def test_block_bits_beyond_the_largest_token():
    b5 = [[hg + 1] * 32 for hg in range(5)]
    v = np.zeros(64, np.int64)
    assert RD.block_bits(v, b5) == 1                     # an EOB at index 0
    v[0], v[63] = 2000, -1
    assert RD.block_bits(v, b5) == 1 + 2 + 5             # token 22 whatever the size; ZRL from index 1; the value; no EOB


# ---- the stream --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,q,delta,k", [(0, 32, 0, 0), (2, 16, 8, 0), (3, 48, 8, 4)], ids=["420", "422-bqi", "444-bqi-mask"])
def test_restatement_packets_decode_to_its_reconstruction(trace_env, fmt, q, delta, k):
    from oracle import ref
    from theora_amd.encoder import Encoder
    w, h = 64, 48
    headers = Encoder(w, h, fmt, q).header_packets()
    setup = enc_ref.SetupParams(headers[2])
    frames = M.sequence("uncover", w, h, fmt, 4, seed=q)
    e = RD.RdEncoder(w, h, fmt, (0, 0, w, h), setup, 64, 6, delta, k)
    packets, recons, wins = [], [], np.zeros(6, int)
    for n, fr in enumerate(frames):
        r = e.frame(fr, q)
        packets.append(r["packet"])
        recons.append(e.recon)
        assert r["rd"]["on"] == 1 and r["rd"]["measured"] == int(n > 0 and bool(r["packet"]))
        if r["rd"]["measured"]:
            wins += np.bincount(r["decision"]["cand"], minlength=6)
            assert r["rd"]["lam"] == RD.rd_lambda(setup.qmat(1, 0, q)[ZIGZAG][1])
    e.close()
    assert (wins > 0).sum() >= 3, wins
    _decode_check(e, headers, packets, recons, w, h, fmt)
    if ref.available():   # the reference decoder too, where it has been built
        rd = ref.RefDecoder(headers)
        for pkt, rec in zip(packets, recons):
            assert rd.packetin(pkt)[0] >= 0
            got = rd.ycbcr_out()
            for p in range(3):
                assert np.array_equal(got[p], rec[p]), p
        rd.close()


def test_switch_off_is_the_eight_mode_restatement(setup64):
    w, h = 64, 48
    frames = M.sequence("uncover", w, h, 0, 3, seed=4)
    a = M.ModesEncoder(w, h, 0, (0, 0, w, h), setup64[1], 64, 6)
    b = RD.RdEncoder(w, h, 0, (0, 0, w, h), setup64[1], 64, 6, rd=False)
    c = RD.RdEncoder(w, h, 0, (0, 0, w, h), setup64[1], 64, 6, modes=False)   # five modes: the switch does nothing
    from tests import enc_inter_ref as IR
    d = IR.InterEncoder(w, h, 0, (0, 0, w, h), setup64[1], 64, 6)
    for fr in frames:
        ra, rb, rc, rd_ = a.frame(fr, 30), b.frame(fr, 30), c.frame(fr, 30), d.frame(fr, 30)
        assert ra["packet"] == rb["packet"] and rb["rd"] == dict(on=0, measured=0, huff=[0] * 4, lam=0)
        assert rc["packet"] == rd_["packet"] and rc["rd"] == dict(on=1, measured=0, huff=[0] * 4, lam=0)
    for e in (a, b, c, d):
        e.close()


def test_the_gpu_packet_cases_are_not_vacuous():
    """Over the case list of tests/test_gpu_encoder_rd.py every candidate wins somewhere, and every case has a macro block whose mode is
    not enc_modes_ref.decide's."""
    from theora_amd.encoder import Encoder
    wins = np.zeros(6, int)
    for case in RD.PACKET_CASES:
        kind, w, h, fmt, q, nf = case
        setup = enc_ref.SetupParams(Encoder(w, h, fmt, q).header_packets()[2])
        e = RD.RdEncoder(w, h, fmt, (0, 0, w, h), setup, 64, 6)
        differ = 0
        for fr in RD.case_frames(case):
            r = e.frame(fr, q)
            if r["rd"]["measured"]:
                d = r["decision"]
                wins += np.bincount(d["cand"], minlength=6)
                differ += int((M.decide(d, int(setup.qmat(1, 0, q)[ZIGZAG][1]))["pix"] != d["pix"]).sum())
        e.close()
        assert differ > 0, case
    print("wins by candidate", wins)
    assert (wins > 0).all(), wins
    assert {c[3] for c in RD.PACKET_CASES} == {0, 2, 3} and {c[4] for c in RD.PACKET_CASES} == {0, 16, 48, 63}
    assert all(64 <= c[1] <= 176 and 48 <= c[2] <= 144 for c in RD.PACKET_CASES)


# ---- what it buys ------------------------------------------------------------------------------------------------------------------
_SWEEPS = {}


def _sweep(setup, name, delta, rd):
    """DESIGN.md section 5.15's inter measurement: per quality (bytes, mean Y window_q20, Y sse) over the two shifted frames coded as
    inter frames with eight modes behind the key frame of picture `name`; block qi delta (0: off), the rule on or off."""
    key = (name, delta, rd)
    if key in _SWEEPS:
        return _SWEEPS[key]
    from tests import picture_compare_ref as PC
    first = _composite() if name == "composite" else _pan()
    frames = [first] + [_shifted(first, *s) for s in SHIFTS]
    rows = []
    for q in QUALITIES:
        e = RD.RdEncoder(W, H, 0, (0, 0, W, H), setup, 64, 6, delta, 0, True, rd)
        nbytes, q20, sse = 0, [], 0
        for n, fr in enumerate(frames):
            r = e.frame(fr, q)
            if n == 0:
                continue
            nbytes += len(r["packet"])
            rec = np.asarray(e.recon[0], np.int64)
            q20.append(PC.window_q20(fr[0], rec).mean())
            sse += int(((np.asarray(fr[0], np.int64) - rec) ** 2).sum())
        e.close()
        rows.append((nbytes, float(np.mean(q20)), sse))
    _SWEEPS[key] = rows
    return rows


# (picture, block-qi delta) -> bytes at matched mean Y SSIM, the rule on against the SAD cascade, as measured with the constants of
# theoraenc_hip.h (DESIGN.md section 5.16 lists the other constants tried).  Only the smooth pan without block qi shows a gain: its
# bound is the midpoint between the measured 0.9700 and 1 (section 5.15's convention).  The other three show none -- 1.0041, 1.0172
# and 1.0012 -- so there is nothing to claim there and the test keeps the record honest: the figure written down, within 0.005.
GAIN_BOUNDS = {("pan", 0): 0.9850}
NO_GAIN_RECORD = {("composite", 0): 1.0041, ("composite", 8): 1.0172, ("pan", 8): 1.0012}


@pytest.mark.parametrize("name,delta", list(GAIN_BOUNDS) + list(NO_GAIN_RECORD))
def test_bytes_at_matched_ssim(setup176, name, delta):
    off, on = _sweep(setup176, name, delta, False), _sweep(setup176, name, delta, True)
    ssim, psnr = _bytes_at_matched(off, on, _ssim), _bytes_at_matched(off, on, _psnr)
    print("\n%s D=%d: bytes at matched Y SSIM %.4f, at matched Y PSNR %.4f" % (name, delta, ssim, psnr))
    print("  off", [(r[0], round(r[1]), r[2]) for r in off])
    print("  on ", [(r[0], round(r[1]), r[2]) for r in on])
    if (name, delta) in GAIN_BOUNDS:
        assert ssim <= GAIN_BOUNDS[(name, delta)], ssim
    else:
        assert abs(ssim - NO_GAIN_RECORD[(name, delta)]) < 0.005, ssim
