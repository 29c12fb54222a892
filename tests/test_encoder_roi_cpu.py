"""Region-of-interest maps (TH_ENCCTL_THIP_SET_ROI_MAP; include/theoraenc_hip.h, "Region of interest") without a GPU: the rule's table
and arithmetic, the restatement tests/enc_roi_ref.py against a scalar loop, what follows from the rule, the refusals of the two
requests and of thip_enc_roi_stage, and the kernel's lane on the host under sanitizers.  The GPU's half: tests/test_gpu_roi_direct.py
and tests/test_gpu_encoder_roi.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from tests import enc_bqi_ref as B
from tests import enc_inter_ref as IR
from tests import enc_mask_ref as K
from tests import enc_rdq_ref as Q
from tests import enc_ref
from tests import enc_roi_ref as R
from tests.enc_ref import ZIGZAG
from tests.test_encoder_bqi_cpu import _ctl, _enc

TH_EFAULT, TH_EINVAL, TH_EIMPL = -1, -10, -23
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOS = [(64, 48, (0, 0, 64, 48)), (80, 64, (5, 3, 67, 49))]
FMTS = [0, 2, 3]


def map_sizes(pic):
    """(Wm, Hm): 1 x 1, 2 x 3, the macro-block grid, the pixel grid, twice the picture, and the longest maps a side allows."""
    pw, ph = pic[2], pic[3]
    return [(1, 1), (2, 3), ((pw + 15) // 16, (ph + 15) // 16), (pw, ph), (2 * pw, 2 * ph), (16384, 1), (1, 16384)]


def random_map(rng, wm, hm):
    return rng.integers(-64, 65, (hm, wm)).astype(np.int8)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_the_table_is_two_to_the_f_sixteenths_in_exact_integers():
    """T[f] = round(2048 2^(f / 16)): T - 1/2 < 2048 2^(f / 16) < T + 1/2, raised to the 16th power so that both sides are integers:
    (2 T - 1)^16 < 2^f 4096^16 < (2 T + 1)^16.  The header's 16 literals, the kernel's and the restatement's are the same."""
    text = open(os.path.join(ROOT, "include", "theoraenc_hip.h")).read()
    m = re.search(r"\n \*\s+T = ((?:\d+, ){15}\d+)\.", text)
    assert m, "the header states T as 16 literals"
    header = [int(v) for v in m.group(1).split(", ")]
    kernel = re.search(r"#define THIP_ROI_T \{([^}]*)\}", open(os.path.join(ROOT, "theora_amd", "csrc", "thip_encode_roi.h")).read())
    assert header == R.T == [int(v) for v in kernel.group(1).split(",")]
    for f, t in enumerate(header):
        assert (2 * t - 1) ** 16 < 2 ** f * 4096 ** 16 < (2 * t + 1) ** 16, f


def exact_r(v):
    """r of a uniform map v, from the definition alone: T by the inequality above, then the shift with its rounding."""
    n = -v
    o, f = n >> 4, n & 15
    t = next(t for t in range(2048, 4097) if (2 * t - 1) ** 16 < 2 ** f * 4096 ** 16 < (2 * t + 1) ** 16)
    return t << o if o >= 0 else (t + (1 << (-o - 1))) >> -o


def test_uniform_maps_give_two_to_the_minus_v_sixteenths():
    geo = IR.Geometry(64, 48, 0)
    for v in range(-64, 65):
        i, st = R.roi_scales(geo, (0, 0, 64, 48), 0, np.full((3, 5), v, np.int8))
        r = exact_r(v)
        assert (i == r).all() and 128 <= r <= 32768, v
        assert abs(r / 2048.0 / 2.0 ** (-v / 16.0) - 1) < 0.004, v   # (the rounding to 1/2048 at the small end: 1 / 256)
        assert st == dict(exp_min=v, exp_max=v, exp_sum=48 * v, scale_min=r, scale_max=r)
    assert exact_r(0) == 2048 and exact_r(64) == 128 and exact_r(-64) == 32768 and exact_r(16) == 1024 and exact_r(-16) == 4096


# ---- the restatement against a scalar loop ----------------------------------------------------------------------------------------
def scalar_scales(fw, fh, fmt, pic, v, mask=None):
    """The rule, sample by sample: (iscale, stats)."""
    hdec, vdec = int(not (fmt & 1)), int(not (fmt & 2))
    px, py, pw, ph = pic
    hm, wm = len(v), len(v[0])
    out, es = [], []
    for p in range(3):
        hd, vd = (hdec, vdec) if p else (0, 0)
        nh, nv = (fw >> 3) >> hd, (fh >> 3) >> vd
        for fy in range(nv):             # rows from the bottom
            for fx in range(nh):
                S = 0
                for r in range(8):
                    Y = (nv - 1 - fy) * 8 + r
                    y = min(max((Y << vd) - py, 0), ph - 1)
                    row = v[y * hm // ph]
                    for c in range(8):
                        x = min(max(((fx * 8 + c) << hd) - px, 0), pw - 1)
                        S += row[x * wm // pw]
                e = (S + 32) >> 6
                n = -e
                o, f = n >> 4, n & 15
                r_ = R.T[f] << o if o >= 0 else (R.T[f] + (1 << (-o - 1))) >> -o
                m = 2048 if mask is None else int(mask[len(out)])
                out.append(min(max((m * r_ + 1024) >> 11, 128), 32768))
                if p == 0:
                    es.append(e)
    return out, dict(exp_min=min(es), exp_max=max(es), exp_sum=sum(es), scale_min=min(out), scale_max=max(out))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("fw,fh,pic", GEOS)
def test_roi_scales_against_the_scalar_loop(fw, fh, pic, fmt):
    geo = IR.Geometry(fw, fh, fmt)
    rng = np.random.default_rng(fw + fmt)
    for k, (wm, hm) in enumerate(map_sizes(pic)):
        v = random_map(rng, wm, hm)
        mask = rng.integers(128, 32769, geo.nfrags) if k & 1 else None
        i, st = R.roi_scales(geo, pic, fmt, v, mask)
        wi, wst = scalar_scales(fw, fh, fmt, pic, v.tolist(), mask)
        assert i.tolist() == wi and st == wst, (wm, hm)
        assert -64 <= st["exp_min"] <= st["exp_max"] <= 64


def test_the_zero_map_gives_maskings_scales():
    fw, fh, pic = 80, 64, (5, 3, 67, 49)
    geo = IR.Geometry(fw, fh, 0)
    rng = np.random.default_rng(2)
    act = rng.integers(0, 1 << 16, geo.planes[0]["nfrags"])
    for k in (2, 4, 16):
        m = K.scales(act, k, geo)[0]
        i, st = R.roi_scales(geo, pic, 0, np.zeros((4, 5), np.int8), m)
        assert (i == m).all() and (st["exp_min"], st["exp_max"], st["exp_sum"]) == (0, 0, 0)
    i, st = R.roi_scales(geo, pic, 0, np.zeros((4, 5), np.int8))
    assert (i == 2048).all() and st["scale_min"] == st["scale_max"] == 2048


def test_the_clamps_are_reached_with_masking_at_sixteen():
    """Masking at k = 16 reaches 128 by itself (activity 0 against a large average) and comes near 32768 the other way round; the map's
    +-4 octaves on top of it pass both ends, and the final scale stays inside."""
    geo = IR.Geometry(64, 48, 0)
    n = geo.planes[0]["nfrags"]
    act = np.full(n, 1 << 20, np.int64)
    act[0] = 0
    m = K.scales(act, 16, geo)[0]
    assert m.min() == 128
    act = np.zeros(n, np.int64)
    act[0] = (1 << 32) - 1
    m2 = K.scales(act, 16, geo)[0]
    assert m2.max() == m2[0] > 16384   # (one busy block among 47 flat ones: 24608; 32768 takes a larger frame)
    lo = R.roi_scales(geo, (0, 0, 64, 48), 0, np.full((1, 1), 64, np.int8), m)[0]
    hi = R.roi_scales(geo, (0, 0, 64, 48), 0, np.full((1, 1), -64, np.int8), m2)[0]
    assert lo.min() == 128 and lo[0] == 128 and (128 * 128 + 1024) >> 11 < 128
    assert hi.max() == 32768 and hi[0] == 32768 and (int(m2[0]) * 32768 + 1024) >> 11 > 32768


# ---- what follows from the rule ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup64():
    from theora_amd.encoder import Encoder
    headers = Encoder(64, 48, 0, 32).header_packets()
    return headers, enc_ref.SetupParams(headers[2])


def test_raising_v_never_raises_a_blocks_ac_distortion(setup64):
    """On a key frame the block takes the least D_k + lambda_b (R_k + flag): the minimiser's D does not fall as lambda_b grows, and
    lambda_b does not grow with v.  Block by block over uniform maps of rising v: the chosen D_k never rises."""
    setup = setup64[1]
    w, h = 64, 48
    planes = IR.sequence("pan", w, h, 0, 1, seed=5)[0]
    src = np.flipud(enc_ref.frame_planes(planes, w, h, 0, (0, 0, w, h))[0]).astype(np.int64)
    r = np.arange(8)
    fy, fx = np.divmod(np.arange(48), 8)
    res = (src[fy[:, None, None] * 8 + r[None, :, None], fx[:, None, None] * 8 + r[None, None, :]] - 128).reshape(-1, 64)
    dct = oracle.fdct8x8_batch(res.astype(np.int16))
    tabs = [setup.qmat(0, 0, q)[ZIGZAG] for q in B.qi_list(32, 12)]
    bits = B.token_bits(setup, 5)
    dist = []
    for tab in tabs:
        q = oracle.quantize_batch(dct, np.asarray(tab, np.uint16))[0].astype(np.int64)
        e = dct.astype(np.int64)[:, 1:] - q[:, 1:] * np.asarray(tab, np.int64)[1:]
        dist.append((e * e).sum(1))
    dist = np.stack(dist, 1)
    geo = IR.Geometry(w, h, 0)
    last, moved = None, 0
    for v in range(-64, 65, 4):
        iscale = R.roi_scales(geo, (0, 0, w, h), 0, np.full((1, 1), v, np.int8))[0][:48]
        qii = K.choose(dct, tabs, bits, iscale)[1]
        d = dist[np.arange(48), qii]
        if last is not None:
            assert (d <= last).all(), v
            moved += int((d < last).sum())
        last = d
    assert moved >= 48   # (not vacuous: on average every block changes its qi at least once on the way)


def test_the_restatement_with_a_zero_map_and_with_block_qi_off_is_the_plain_stream(setup64):
    setup = setup64[1]
    w, h = 64, 48
    frames = IR.sequence("pan", w, h, 0, 2, seed=4)
    rng = np.random.default_rng(9)
    busy = random_map(rng, 4, 3)
    for delta, k, roi in ((8, 0, np.zeros((3, 4), np.int8)), (8, 4, np.zeros((1, 1), np.int8)), (0, 0, busy), (0, 4, busy)):
        a = R.RoiEncoder(w, h, 0, (0, 0, w, h), setup, 64, 6, delta, k, True, False, True, 3)
        b = Q.RdqEncoder(w, h, 0, (0, 0, w, h), setup, 64, 6, delta, k, True, False, True, 3)
        for f in frames:
            x, y = a.frame(f, 32, roi=roi), b.frame(f, 32)
            assert x["packet"] == y["packet"] and x["mask"] == y["mask"], (delta, k)
            assert x["roi"]["measured"] == int(bool(delta)) and x["roi"]["active"] == 1
        a.close()
        b.close()
    # and a map that is not zero moves the packets, with masking and without it
    for k in (0, 4):
        a = R.RoiEncoder(w, h, 0, (0, 0, w, h), setup, 64, 6, 8, k, True, False, True, 3)
        b = Q.RdqEncoder(w, h, 0, (0, 0, w, h), setup, 64, 6, 8, k, True, False, True, 3)
        diff = 0
        for f in frames:
            x, y = a.frame(f, 32, roi=busy), b.frame(f, 32)
            diff += x["packet"] != y["packet"]
            assert x["roi"]["measured"] == 1 and x["mask"]["ratio"] == k and x["mask"]["measured"] == int(bool(k))
        assert diff == 2, k
        assert K.scales.__module__ == "tests.enc_mask_ref" and a.k == k   # (the source is back in its place)
        a.close()
        b.close()


def halves_sse(setup, delta, roi):
    """(bytes, luma SSE of the left half, of the right half) of the 176 x 144 "pan" key frame at quality 32 in the restatement."""
    w, h = 176, 144
    planes = IR.sequence("pan", w, h, 0, 1, seed=21)[0]
    e = R.RoiEncoder(w, h, 0, (0, 0, w, h), setup, 1, 6, delta, 0, False, False, False, 0)
    out = e.frame(planes, 32, roi=roi)
    d = (e.recon[0].astype(np.int64) - planes[0].astype(np.int64)) ** 2
    e.close()
    return len(out["packet"]), int(d[:, :w // 2].sum()), int(d[:, w // 2:].sum())


def test_the_picture_moves_the_way_the_map_says():
    """tests/test_gpu_encoder_roi.py's picture test, on the restatement first: the left half at v = +32 loses luma SSE and the right
    half at -32 gains it, at delta 12 on the 176 x 144 "pan" key frame at quality 32."""
    from theora_amd.encoder import Encoder
    setup = enc_ref.SetupParams(Encoder(176, 144, 0, 32).header_packets()[2])
    roi = np.concatenate([np.full((1, 1), 32, np.int8), np.full((1, 1), -32, np.int8)], 1)
    off, on = halves_sse(setup, 12, None), halves_sse(setup, 12, roi)
    print("\nwithout the map: %d bytes, SSE left %d right %d; with it: %d bytes, left %d right %d" % (off + on))
    assert on[1] < off[1] and on[2] > off[2]


# ---- the controls, on the host library ---------------------------------------------------------------------------------------------
def _roi_map(E, data=None, **kw):
    a = E.RoiMap()
    a.width, a.height, a.device, a.pitch = 4, 3, 0, 4
    if data is not None:
        a.map = data.ctypes.data
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_roi_controls_refuse_before_a_device_is_touched():
    """The refusals of both requests; none touches the GPU (this machine may have none; a good map would: tests/test_gpu_encoder_roi.py).
    The numbers left free stay unknown requests."""
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_SET_ROI_MAP, E.TH_ENCCTL_THIP_GET_ROI_STATS) == (0x7225, 0x7226)
    assert C.sizeof(E.RoiMap) == 40 and C.sizeof(E.RoiStats) == 56
    L, enc = _enc()
    try:
        s = E.RoiStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_ROI_STATS, C.byref(s), C.sizeof(s)) == 0   # before any packet
        assert all(getattr(s, k) == 0 for k, _ in E.RoiStats._fields_)
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_ROI_STATS, C.byref(s), C.sizeof(s) - 8) == TH_EINVAL
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_ROI_STATS, None, C.sizeof(s)) == TH_EINVAL
        good = np.zeros((3, 4), np.int8)
        SET = E.TH_ENCCTL_THIP_SET_ROI_MAP
        assert L.th_encode_ctl(enc, SET, None, 40) == TH_EFAULT
        a = _roi_map(E, good)
        assert L.th_encode_ctl(enc, SET, C.byref(a), 32) == TH_EINVAL
        assert L.th_encode_ctl(enc, SET, C.byref(a), 48) == TH_EINVAL
        for kw in (dict(width=0), dict(width=-1), dict(width=16385), dict(height=0), dict(height=16385), dict(height=-(1 << 31)),
                   dict(pitch=3), dict(pitch=-3), dict(pitch=0), dict(device=2), dict(device=-1)):
            a = _roi_map(E, good, **kw)
            assert L.th_encode_ctl(enc, SET, C.byref(a), C.sizeof(a)) == TH_EINVAL, kw
        for bad in (65, -65, 127, -128):
            for at in ((0, 0), (2, 3), (1, 2)):
                m = np.zeros((3, 8), np.int8)
                m[:, 4:] = 100          # (the padding is not the map's)
                m[at] = bad
                a = _roi_map(E, m, pitch=8)
                assert L.th_encode_ctl(enc, SET, C.byref(a), C.sizeof(a)) == TH_EINVAL, (bad, at)
        m = np.zeros((3, 4), np.int8)
        m[0, 1] = 70                    # row 0 of a map with a negative pitch is the last in memory
        a = _roi_map(E, m, pitch=-4)
        a.map = m.ctypes.data + 8
        assert L.th_encode_ctl(enc, SET, C.byref(a), C.sizeof(a)) == TH_EINVAL
        a = _roi_map(E)                 # no map: cleared, whatever the other fields say
        a.width = -5
        assert L.th_encode_ctl(enc, SET, C.byref(a), C.sizeof(a)) == 0
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_ROI_STATS, C.byref(s), C.sizeof(s)) == 0 and s.active == 0
        for free in (0x7216, 0x7217, 0x721A, 0x7220, 0x7221, 0x7224):
            assert _ctl(L, enc, free, 0)[0] == TH_EIMPL, hex(free)
            assert L.th_encode_ctl(enc, free, C.byref(a), C.sizeof(a)) == TH_EIMPL, hex(free)
    finally:
        L.th_encode_free(enc)


def test_python_encoder_set_roi_arguments():
    from theora_amd.encoder import Encoder
    e = Encoder(64, 48, 0, 20, block_qi=8)
    zero = dict(active=0, measured=0, map_width=0, map_height=0, exp_min=0, exp_max=0, exp_sum=0, scale_min=0, scale_max=0, clamped=0,
                roi_ms=0.0)
    assert e.roi_stats() == zero
    e.set_roi(None)
    assert e.roi_stats() == zero
    for bad in (np.zeros((2, 2), np.int16), np.zeros((2, 2), np.uint8), [[0, 1]], "map"):
        with pytest.raises(TypeError):
            e.set_roi(bad)
    for bad in (np.zeros(4, np.int8), np.zeros((2, 2, 2), np.int8), np.zeros((0, 3), np.int8), np.zeros((2, 2, 1), np.float32)):
        with pytest.raises(ValueError):
            e.set_roi(bad)
    with pytest.raises(ValueError):
        e.set_roi(np.full((2, 2), 65, np.int8))       # a host entry out of range
    with pytest.raises(ValueError):
        e.set_roi(np.zeros((1, 16385), np.int8))
    assert e.roi_stats() == zero
    assert e.header_packets() == Encoder(64, 48, 0, 20).header_packets()
    e.close()
    x = np.array([[-5.0, -4.0, -0.03126, -0.03125, 0.0, 0.09, 0.1, 3.97, 4.0, 9.0]])
    assert R.from_octaves(x).tolist() == [[-64, -64, -1, 0, 0, 1, 2, 64, 64, 64]]


def test_roi_stage_refusals():
    """Every refusal of thip_enc_roi_stage comes before a device is touched: the pointers are never followed."""
    from theora_amd import _lib
    from theora_amd import encoder as E
    EFAULT, EINVAL = _lib.EFAULT, _lib.EINVAL
    L = _lib.load()
    assert L.thip_enc_roi_stage(None) == EFAULT
    assert C.sizeof(_lib.EncRoiReq) == 80
    good = dict(frame=(80, 64), pixel_fmt=0, map_size=(5, 4), map_pitch=8, map=0x1001, pic=(5, 3, 67, 49), mask_iscale=0x2000,
                iscale=0x3000, stats=0x4000)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return E.roi_stage(a.pop("frame"), a.pop("pixel_fmt"), a.pop("map_size"), a.pop("map_pitch"), a.pop("map"), **a)
    for kw in (dict(map=None), dict(iscale=None), dict(stats=None)):
        assert call(**kw) == EFAULT, kw
    for kw in (dict(frame=(0, 64)), dict(frame=(80, 0)), dict(frame=(72, 64)), dict(frame=(80, 60)), dict(frame=(1 << 20, 64)),
               dict(frame=(-16, 64)), dict(frame=(65536, 65536), pic=(0, 0, 16, 16)), dict(pixel_fmt=1), dict(pixel_fmt=4),
               dict(pixel_fmt=-1), dict(pic=(0, 0, 0, 49)), dict(pic=(0, 0, 67, 0)), dict(pic=(-1, 3, 67, 49)), dict(pic=(5, -1, 67, 49)),
               dict(pic=(14, 3, 67, 49)), dict(pic=(5, 16, 67, 49)), dict(pic=(0, 0, 81, 49)), dict(map_size=(0, 4)), dict(map_size=(5, 0)),
               dict(map_size=(16385, 4)), dict(map_size=(5, 16385)), dict(map_size=(-1, 4)), dict(map_pitch=4), dict(map_pitch=-4),
               dict(map_pitch=0), dict(mask_iscale=0x2001), dict(iscale=0x3001), dict(stats=0x4004)):
        assert call(**kw) == EINVAL, kw
    # (a good request, with or without masking's scales: those calls would reach the device)


# ---- the kernel's lane on the host ------------------------------------------------------------------------------------------------
def test_kernel_lane_on_the_host_stays_inside_the_map(tmp_path):
    """k_enc_roi_scale's lane runs fragment by fragment on the host under AddressSanitizer and UBSan (tests/native/roi_scale_host.cpp):
    no load is anything but an entry of the map -- the padding between rows is poisoned --, no store leaves the output, and every
    scale and exponent equals a sample-by-sample restatement of the rule: three geometries, three pixel formats, map widths and heights
    round every switch between the coarse, dword and byte paths, odd bases, tight, padded and negative pitches, with and without
    masking's scales, both widths of the cell arithmetic, and the longest maps a side allows."""
    exe = str(tmp_path / "roi_scale_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused",
           "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "theora_amd", "csrc"), os.path.join(ROOT, "tests", "native", "roi_scale_host.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok: 12963 cases"), (r.stdout[-500:], r.stderr[-3000:])
