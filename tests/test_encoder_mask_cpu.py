"""th_encode_*'s activity masking without a GPU: the rule (include/theoraenc_hip.h, "Activity masking") against exact fractions, the
restatement (tests/enc_mask_ref.py) against the block-qi restatement it extends and against the oracle's decode of its own packets,
the controls (TH_ENCCTL_THIP_SET_MASKING, TH_ENCCTL_THIP_GET_MASK_STATS) and thip_enc_mask_stage's refusals on the host library,
and what masking buys: bytes at matched SSIM against block qi alone.  Nothing here reaches a device."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import oracle
from tests import enc_bqi_ref as B
from tests import enc_inter_ref as IR
from tests import enc_mask_ref as K
from tests import enc_modes_ref as M
from tests import enc_ref
from tests import picture_compare_ref as PC
from tests.test_encoder_bqi_cpu import _ctl, _decode_check, _enc, trace_env   # noqa: F401  (trace_env: a fixture)

TH_EINVAL, TH_EIMPL = -10, -23
PF_420 = 0


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def _half_up(fr):
    return (2 * fr.numerator + fr.denominator) // (2 * fr.denominator)


@pytest.mark.parametrize("k", [2, 4, 16])
def test_scale_rule_against_exact_fractions(k):
    acts = [0, 1, 63, 64, 65, 4095, 5 << 12, (8 << 12) - 1, 8 << 12, 100000, 1 << 24, (1 << 28) + 12345, (1 << 32) - 1]
    avgs = [64, 65, 1000, 5 << 12, 33333, 1 << 20, (1 << 28) + 7]
    for A in avgs:
        last = None
        for a in sorted(set(acts + [A])):
            i = K.luma_scale(a, A, k)
            exact = Fraction(2048 * (k * a + A), a + k * A)
            assert i == _half_up(exact), (a, A, k, i)          # round half up, exactly
            assert 2048 // k <= i <= 2048 * k, (a, A, k, i)
            if a == A:
                assert i == 2048
            assert last is None or i >= last, (a, A, k)   # monotone in a
            last = i
        assert K.luma_scale(0, A, k) == 2048 // k and K.luma_scale((1 << 32) - 1, 64, k) in (2048 * k - 1, 2048 * k)
    # the vector form (scales) is the scalar form
    class G:
        planes = [dict(nhfrags=2, nfrags=4)]
        nfrags, nmbx, mb_of = 4, 1, np.zeros(4, np.int64)
    act = np.array([0, 5 << 12, 1 << 20, (1 << 32) - 1], np.int64)
    got, A, amax = K.scales(act, k, G)
    assert A == K.average(act) and amax == (1 << 32) - 1
    assert got.tolist() == [K.luma_scale(a, A, k) for a in act.tolist()]


def test_average_floor_and_rounding():
    assert K.average(np.zeros(6, np.int64)) == 64
    assert K.average(np.array([64, 65], np.int64)) == 65          # (129 + 1) / 2
    assert K.average(np.array([100, 101, 101], np.int64)) == 101  # (302 + 1) / 3 = 101
    assert K.average(np.array([100, 100, 101], np.int64)) == 100  # (301 + 1) / 3 = 100


def test_chroma_rule_on_all_orderings():
    for vals, want in (((3000, 2500, 2100, 2049), 2049),     # none under 2048: the least
                       ((3000, 2500, 2100, 1000), 2100),     # one flat block is ignored
                       ((3000, 2500, 1500, 1000), 2048),     # two: the second least, floored
                       ((900, 800, 700, 600), 2048),
                       ((2048, 2048, 2048, 2048), 2048),
                       ((2048, 4000, 5000, 512), 2048),      # the second least is 2048 itself
                       ((4000, 4000, 4000, 2047), 4000)):
        for perm in itertools.permutations(vals):
            assert K.chroma_scale(perm) == want, perm


# ---- the choice --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup64():
    from theora_amd.encoder import Encoder
    headers = Encoder(64, 48, 0, 32).header_packets()
    return headers, enc_ref.SetupParams(headers[2])


def test_choice_at_unit_scale_is_block_qis(setup64):
    setup = setup64[1]
    rng = np.random.default_rng(11)
    bits = B.token_bits(setup, 5)
    for qis, t, p in (([32, 24, 40], 0, 0), ([10, 2], 1, 1), ([60, 48, 63], 0, 2)):
        res = (rng.normal(0, rng.choice([2, 12, 40], (96, 1)), (96, 64))).astype(np.int16)
        dct = oracle.fdct8x8_batch(res)
        tabs = [setup.qmat(t, p, q)[enc_ref.ZIGZAG] for q in qis]
        want = B.choose(dct, tabs, bits)
        got = K.choose(dct, tabs, bits, np.full(96, 2048))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert len(set(want[1].tolist())) > 1


def test_a_block_whose_choice_flips_with_the_scale():
    """One coefficient c = 24 at zig-zag index 1; steps 16 at qis[0] and 8 at qis[1]; every token costs 4 bits.  Levels 2 (24 / 16
    rounds to 2: error 8) and 3 (error 0), both one token and an EOB: D = 64 or 0, R = 8 either way, and qis[1] pays one lambda more
    for its flag.  lambda = 16 * 16 * 40 >> 7 = 80: at scale 512 lambda_b = 20 < 64 and the block takes qis[1]; at 8192 lambda_b
    = 320 > 64 and it stays at qis[0]."""
    dct = np.zeros((1, 64), np.int16)
    dct[0, 1] = 24
    tabs = [np.full(64, 16, np.uint16), np.full(64, 8, np.uint16)]
    bits = [[4] * 32 for _ in range(4)]
    q0 = oracle.quantize_batch(dct, tabs[0])[0][0, 1]
    q1 = oracle.quantize_batch(dct, tabs[1])[0][0, 1]
    assert (int(q0), int(q1)) == (2, 3)
    lo = K.choose(dct, tabs, bits, np.array([512]))
    hi = K.choose(dct, tabs, bits, np.array([8192]))
    assert lo[1].tolist() == [1] and lo[0][0, 1] == 3
    assert hi[1].tolist() == [0] and hi[0][0, 1] == 2


# ---- the activity ------------------------------------------------------------------------------------------------------------------
def test_activity_over_an_odd_picture_region():
    fw, fh, pic = 80, 64, (5, 3, 67, 49)
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, (fh, fw)).astype(np.uint8), np.full((fh // 2, fw // 2), 128, np.uint8), np.full((fh // 2, fw // 2), 128, np.uint8)]
    got = K.activity(planes, fw, fh, PF_420, pic)
    fp = enc_ref.frame_planes(planes, fw, fh, PF_420, pic)
    want = oracle.mb_cost_maps([np.flipud(a) for a in fp], fw, fh, PF_420)[2]
    nh, nv = fw >> 3, fh >> 3
    assert got.shape == (nh * nv,)
    # block by block, through the reference's own numbering: macro block (super block << 2 | quadrant), entry of its sb_map;
    # the table is a Hilbert curve over the super block's 4 x 4 blocks
    nsbw = (nh + 3) >> 2
    hil = {}
    for sy in range(4):
        for sx in range(4):
            h = int(K.HILBERT[sy, sx])
            hil[h] = (sy, sx)
    assert sorted(hil) == list(range(16))                       # a permutation
    for h in range(15):                                         # a curve: consecutive places are neighbours
        assert abs(hil[h][0] - hil[h + 1][0]) + abs(hil[h][1] - hil[h + 1][1]) == 1
    for by in range(nv):
        for bx in range(nh):
            h = int(K.HILBERT[by & 3, bx & 3])
            mbi = (((by >> 2) * nsbw + (bx >> 2)) << 2) | (h >> 2)
            assert got[by * nh + bx] == want[mbi, h & 3]
    # flipping the frame moves the values and changes none: rows from the top give the same map, upside down
    top = K.luma_raster(oracle.mb_cost_maps(fp, fw, fh, PF_420)[2], fw, fh)
    assert np.array_equal(top[::-1].reshape(-1), got)
    # the clamp matters: the same planes with the padding zeroed give another map
    zeroed = [a.copy() for a in fp]
    mask = np.zeros((fh, fw), bool)
    mask[3:3 + 49, 5:5 + 67] = True
    zeroed[0][~mask] = 0
    other = K.luma_raster(oracle.mb_cost_maps([np.flipud(a) for a in zeroed], fw, fh, PF_420)[2], fw, fh).reshape(-1)
    assert (other != got).any()
    # and a frame-size input is read through the region alone
    junk = [a.copy() for a in planes]
    junk[0][~mask] = 255 - junk[0][~mask]
    assert np.array_equal(K.activity(junk, fw, fh, PF_420, pic), got)


# ---- the stream --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,delta,k,nqis", [(32, 8, 2, 3), (0, 6, 16, 2), (63, 10, 2, 2), (60, 12, 16, 3)])
@pytest.mark.parametrize("kind", ["key", "five", "eight"])
def test_restatement_packets_decode_to_its_reconstruction(trace_env, setup64, kind, q, delta, k, nqis):
    from oracle import ref
    w, h, fmt = 64, 48, 0
    headers, setup = setup64
    frames = M.sequence("shear" if kind == "eight" else "pan", w, h, fmt, 4, seed=q + delta)
    e = K.MaskEncoder(w, h, fmt, (0, 0, w, h), setup, 1 if kind == "key" else 64, 6, delta, k, modes=kind == "eight")
    packets, recons = [], []
    for fr in frames:
        r = e.frame(fr, q)
        packets.append(r["packet"])
        recons.append(e.recon)
        if r["packet"]:
            assert r["bqi"]["nqis"] == nqis and r["bqi"]["qis"][:nqis] == B.qi_list(q, delta)
            assert r["mask"]["measured"] == 1 and r["mask"]["ratio"] == k and r["mask"]["activity_avg"] >= 64
        else:
            assert r["mask"] == dict(ratio=k, measured=0, activity_avg=0, activity_max=0)
    e.close()
    _decode_check(e, headers, packets, recons, w, h, fmt)
    if ref.available():   # the reference decoder too, where it has been built
        rd = ref.RefDecoder(headers)
        for pkt, rec in zip(packets, recons):
            assert rd.packetin(pkt)[0] >= 0
            got = rd.ycbcr_out()
            for p in range(3):
                assert np.array_equal(got[p], rec[p]), p
        rd.close()


def test_masking_off_is_the_block_qi_restatement(setup64):
    w, h = 64, 48
    frames = IR.sequence("pan", w, h, 0, 2, seed=4)
    for delta, k in ((8, 0), (0, 4)):
        a = B.BqiEncoder(w, h, 0, (0, 0, w, h), setup64[1], 64, 6, delta)
        b = K.MaskEncoder(w, h, 0, (0, 0, w, h), setup64[1], 64, 6, delta, k)
        for fr in frames:
            ra, rb = a.frame(fr, 30), b.frame(fr, 30)
            assert ra["packet"] == rb["packet"] and rb["mask"]["measured"] == 0 and rb["mask"]["ratio"] == k
        a.close()
        b.close()


# ---- the controls, on the host library ---------------------------------------------------------------------------------------------
def test_masking_controls():
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_SET_MASKING, E.TH_ENCCTL_THIP_GET_MASK_STATS) == (0x7214, 0x7215)
    assert C.sizeof(E.MaskStats) == 32
    L, enc = _enc()
    try:
        s = E.MaskStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_MASK_STATS, C.byref(s), C.sizeof(s)) == 0   # before any packet
        assert (s.ratio, s.measured, s.activity_avg, s.activity_max, s.mask_ms) == (0, 0, 0, 0, 0.0)
        for k in [0] + list(range(2, 17)) + [0, 4]:
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_MASKING, k) == (0, k)
        for k in (-1, 1, 17, 64, 1 << 20, -(1 << 31)):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_MASKING, k)[0] == TH_EINVAL, k
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_MASKING, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_MASKING, 4, C.c_int64)[0] == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_MASK_STATS, C.byref(s), C.sizeof(s)) == 0
        assert (s.ratio, s.measured) == (4, 0)                                # accepted with block qi off; the ratio in force
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_MASK_STATS, C.byref(s), C.sizeof(s) - 8) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_MASK_STATS, None, C.sizeof(s)) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, 8) == (0, 8)
        assert _ctl(L, enc, 0x7216, 0)[0] == TH_EIMPL                         # the next number is still free
    finally:
        L.th_encode_free(enc)


def test_python_encoder_masking():
    from theora_amd.encoder import Encoder
    e = Encoder(64, 48, 0, 20, block_qi=8, masking=4)
    assert e.masking == 4 and e.mask_stats() == dict(ratio=4, measured=0, activity_avg=0, activity_max=0, mask_ms=0.0)
    e.set_masking(0)
    assert e.mask_stats()["ratio"] == 0
    assert e.header_packets() == Encoder(64, 48, 0, 20).header_packets()
    e.close()
    for bad in (1, 17, -3):
        with pytest.raises(ValueError):
            Encoder(64, 48, 0, 20, masking=bad)


def test_mask_stage_refusals():
    """Every refusal of thip_enc_mask_stage comes before a device is touched: the pointers are never followed."""
    from theora_amd import _lib
    from theora_amd import encoder as E
    EFAULT, EINVAL = _lib.EFAULT, _lib.EINVAL
    L = _lib.load()
    assert L.thip_enc_mask_stage(None) == EFAULT
    assert C.sizeof(_lib.EncMaskReq) == 104
    good = dict(frame=(80, 64), pixel_fmt=0, ratio=4, pic=(5, 3, 67, 49), src=[0x1000, 0x2000, 0x3000], src_pitch=[67, 34, 34],
                act=0x4000, avg=0x5000, iscale=0x6000)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return E.mask_stage(a.pop("frame"), a.pop("pixel_fmt"), a.pop("ratio"), **a)
    for kw in (dict(src=None), dict(src=[0x1000, None, 0x3000]), dict(src=[None, 0x2000, 0x3000]), dict(act=None), dict(avg=None),
               dict(iscale=None)):
        assert call(**kw) == EFAULT, kw
    for kw in (dict(frame=(0, 64)), dict(frame=(80, 0)), dict(frame=(72, 64)), dict(frame=(80, 60)), dict(frame=(1 << 20, 64)),
               dict(frame=(-16, 64)), dict(frame=(65536, 65536), pic=(0, 0, 16, 16)), dict(pixel_fmt=1), dict(pixel_fmt=4),
               dict(pixel_fmt=-1), dict(pic=(0, 0, 0, 49)), dict(pic=(0, 0, 67, 0)), dict(pic=(-1, 3, 67, 49)), dict(pic=(5, -1, 67, 49)),
               dict(pic=(14, 3, 67, 49)), dict(pic=(5, 16, 67, 49)), dict(pic=(0, 0, 81, 49)), dict(src_pitch=[66, 34, 34]),
               dict(src_pitch=[67, 33, 34]), dict(src_pitch=[67, 34, 0]), dict(ratio=0), dict(ratio=1), dict(ratio=17), dict(ratio=-4),
               dict(act=0x4002), dict(avg=0x5004), dict(iscale=0x6001)):
        assert call(**kw) == EINVAL, kw


# ---- what it buys ------------------------------------------------------------------------------------------------------------------
W, H = 176, 144
QUALITIES = (16, 24, 32, 40, 48)
SHIFTS = ((3, 1), (4, -2))


def _composite():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:144, 0:176]
    Y = 60 + xx * 0.5 + yy * 0.3 + rng.normal(0, 1.5, (144, 176))
    Y[:, 88:] = 128 + rng.normal(0, 28, (144, 88))
    Y[72:, :88] += 6 * np.sin(xx[72:, :88] * 0.9) * np.sin(yy[72:, :88] * 0.7)
    return [np.clip(Y, 0, 255).astype(np.uint8),
            np.full((72, 88), 120, np.uint8) + rng.integers(0, 6, (72, 88)).astype(np.uint8),
            np.full((72, 88), 130, np.uint8)]


def _pan():
    return IR.sequence("pan", W, H, 0, 1, seed=21)[0]


def _shifted(planes, dx, dy):
    """The picture moved by (dx, dy) luma pixels, the edge repeated (chroma by half of it, rounded down)."""
    out = []
    for p, a in enumerate(planes):
        sx, sy = (dx, dy) if p == 0 else (dx >> 1, dy >> 1)
        h, w = a.shape
        out.append(a[np.clip(np.arange(h) - sy, 0, h - 1)][:, np.clip(np.arange(w) - sx, 0, w - 1)])
    return out


@pytest.fixture(scope="module")
def setup176():
    from theora_amd.encoder import Encoder
    return enc_ref.SetupParams(Encoder(W, H, 0, 32).header_packets()[2])


_SWEEPS = {}


def _sweep(setup, name, k, inter):
    """Per quality: (bytes, mean Y window_q20, Y sse, qii of the key frame in coded order) of the picture `name` -- its key frame,
    or (inter) its two shifted frames coded as inter frames with eight modes behind it, bytes and metrics over those two."""
    key = (name, k, inter)
    if key in _SWEEPS:
        return _SWEEPS[key]
    first = _composite() if name == "composite" else _pan()
    frames = [first] + ([_shifted(first, *s) for s in SHIFTS] if inter else [])
    rows = []
    for q in QUALITIES:
        e = K.MaskEncoder(W, H, 0, (0, 0, W, H), setup, 64 if inter else 1, 6, 8, k, modes=inter)
        nbytes, q20, sse, qii = 0, [], 0, None
        for n, fr in enumerate(frames):
            r = e.frame(fr, q)
            if n == 0:
                qii = r["qii"]
            if inter and n == 0:
                continue
            nbytes += len(r["packet"])
            rec = np.asarray(e.recon[0], np.int64)
            q20.append(PC.window_q20(fr[0], rec).mean())
            sse += int(((np.asarray(fr[0], np.int64) - rec) ** 2).sum())
        e.close()
        rows.append((nbytes, float(np.mean(q20)), sse, qii))
    _SWEEPS[key] = rows
    return rows


def _bytes_at_matched(off, on, quality):
    """The on/off byte ratio at the qualities both sweeps reach: log-bytes interpolated over the quality, averaged over the overlap
    (tests/test_gpu_encoder_bqi.py's _bytes_at_matched_psnr)."""
    po, bo = np.array([quality(r) for r in off]), np.log(np.array([r[0] for r in off], np.float64))
    pn, bn = np.array([quality(r) for r in on]), np.log(np.array([r[0] for r in on], np.float64))
    lo, hi = max(po.min(), pn.min()), min(po.max(), pn.max())
    ps = np.linspace(lo, hi, 16)
    return float(np.exp(np.mean(np.interp(ps, pn, bn) - np.interp(ps, po, bo))))


def _ssim(r):
    return r[1]


def _psnr(r):
    return -np.log10(max(r[2], 1))   # (monotone in the PSNR; the sample count is the same on both sides)


def test_masking_is_not_vacuous(setup176):
    """On the composite at quality 16 and 32, D = 8, k = 4, at least 5 % of the coded blocks take another qii than block qi alone
    gives them (measured: 18 % and 37 %)."""
    off, on = _sweep(setup176, "composite", 0, False), _sweep(setup176, "composite", 4, False)
    for q in (16, 32):
        a, b = off[QUALITIES.index(q)][3], on[QUALITIES.index(q)][3]
        changed = int((np.asarray(a) != np.asarray(b)).sum())
        print("quality %d: %d of %d blocks change their qii" % (q, changed, len(a)))
        assert changed * 20 >= len(a), (q, changed, len(a))


# (picture, inter) -> the bound on bytes at matched mean Y SSIM, masking on against block qi alone.  Key frames: on the composite the
# midpoint between the measured 0.9534 and 1 ("half the gain", as test_block_qi_lowers_the_cost takes its margin), on the smooth
# pan 1.01 (masking may not cost more than 1 %; measured 0.9970).
KEY_BOUNDS = {"composite": 0.9767, "pan": 1.01}
# Two inter frames with eight modes behind the key frame, bytes and SSIM over those two: masking shows NO gain there (DESIGN.md
# section 5.15 says why) -- measured 1.1993 on the composite and 1.0121 on the pan.  There is nothing to claim, so the test only
# keeps the record honest: the figure is the one written down, within 0.005.
INTER_RECORD = {"composite": 1.1993, "pan": 1.0121}


@pytest.mark.parametrize("name", list(KEY_BOUNDS))
@pytest.mark.parametrize("inter", [False, True], ids=["key", "inter"])
def test_masking_lowers_the_bytes_at_matched_ssim(setup176, name, inter):
    off, on = _sweep(setup176, name, 0, inter), _sweep(setup176, name, 4, inter)
    ssim, psnr = _bytes_at_matched(off, on, _ssim), _bytes_at_matched(off, on, _psnr)
    print("\n%s %s: bytes at matched Y SSIM %.4f, at matched Y PSNR %.4f" % (name, "inter" if inter else "key", ssim, psnr))
    print("  off", [(r[0], round(r[1]), r[2]) for r in off])
    print("  on ", [(r[0], round(r[1]), r[2]) for r in on])
    if inter:
        assert abs(ssim - INTER_RECORD[name]) < 0.005, ssim
    else:
        assert ssim <= KEY_BOUNDS[name], ssim
