"""Picture metrics (thip_picture_compare) without a GPU: the numpy restatement of the definition (tests/picture_compare_ref.py)
against values worked out by hand, the stated bounds of the integer SSIM and its distance from the real-valued one, the kernel's
load-and-sum body run on the host under sanitizers, and the argument checks that return before any state is touched."""
import ctypes as C

import numpy as np
import pytest

from tests import picture_compare_ref as cr

ONE = 1 << 20


def _terms(s, r):
    """a, b, c, d, q1, q2, w of one 8x8 window pair as Python ints."""
    return tuple(int(v.item()) for v in cr.window_terms(*cr.window_sums(s, r)))


def test_equal_planes_by_hand():
    """Equal planes: no squared difference, and every window is exactly 1.0: a = b and c = d, so q1 = q2 = 2^20 and w = 2^20."""
    s = np.random.default_rng(1).integers(0, 256, (21, 30), dtype=np.uint8)
    rec = cr.compare_planes([s, s[:9, :9], s[:8, :8]], [s, s[:9, :9], s[:8, :8]], cr.SSE | cr.SSIM)
    assert rec[0:3] == [0, 0, 0] and rec[3:6] == [21 * 30, 81, 64]
    assert (cr.window_q20(s, s) == ONE).all()
    assert rec[9:12] == [4 * 6, 1, 1] and rec[6:9] == [24 * ONE, ONE, ONE]
    assert (cr.block_sse(s, s) == 0).all() and cr.block_sse(s, s).shape == (3, 4)


def test_black_against_white_by_hand():
    """0 against 255 over one window: sx = 0, sy = 64 * 255 = 16320, sxx = sxy = 0, syy = 64 * 255^2.  a = C1, b = 16320^2 + C1,
    c = C2 (the covariance term is 0), d = 64 syy - sy^2 + C2 = C2 (a flat plane has no variance): q2 = 2^20, w = q1."""
    s, r = np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8)
    a, b, c, d, q1, q2, w = _terms(s, r)
    assert (a, b, c, d) == (26634, 16320 * 16320 + 26634, 239708, 239708)
    assert q1 == (26634 << 20) // b and q2 == ONE and w == q1 == 104
    rec = cr.compare_planes([s] * 3, [r] * 3, cr.SSE | cr.SSIM)
    assert rec[0:3] == [64 * 255 * 255] * 3 and rec[3:6] == [64] * 3 and rec[6:9] == [104] * 3 and rec[9:12] == [1] * 3
    # the GPU suite's 64-bit case: 264 x 256 samples of 255^2
    assert 264 * 256 * 255 * 255 == 4394649600 > 1 << 32


def test_one_sample_lands_in_its_block_and_windows():
    """One sample off by 10 at column 13, row 6 of a 24 x 16 plane: block (1, 0) holds 100, every other block 0; the windows that
    contain it start at columns 8 and 12 (8 <= 13 < 16, 12 <= 13 < 20; 4 ends at 11) and rows 0 and 4: those four are below 2^20,
    the other eleven exactly 2^20."""
    s = np.full((16, 24), 100, np.uint8)
    r = s.copy()
    r[6, 13] = 110
    b = cr.block_sse(s, r)
    assert b.shape == (2, 3) and b[0, 1] == 100 and b.sum() == 100
    w = cr.window_q20(s, r)
    assert w.shape == (3, 5)
    hit = np.zeros((3, 5), bool)
    hit[0:2, 2:4] = True
    assert (w[~hit] == ONE).all() and (w[hit] < ONE).all() and (w[hit] > 0).all()
    assert cr.compare_planes([s] * 3, [r] * 3)[0:3] == [100] * 3


@pytest.mark.parametrize("extent,count", [(7, 0), (8, 1), (11, 1), (12, 2), (13, 2)])
def test_window_count(extent, count):
    s = np.zeros((extent, 16), np.uint8)
    assert cr.window_q20(s, s).shape == (count, 3)
    assert cr.window_q20(s.T, s.T).shape == (3, count)
    rec = cr.compare_planes([s] * 3, [s] * 3, cr.SSIM)
    assert rec[9:12] == [3 * count] * 3 and rec[0:6] == [0] * 6          # (no THIP_CMP_SSE: its fields stay 0)


def _windows(seed, n):
    """n window pairs of each kind: random, near-equal, inverted, flat, and extreme two-level patterns."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = rng.integers(0, 256, (8, 8), dtype=np.uint8)
        out.append((s, rng.integers(0, 256, (8, 8), dtype=np.uint8)))
        out.append((s, np.clip(s.astype(int) + rng.integers(-3, 4, (8, 8)), 0, 255).astype(np.uint8)))
        out.append((s, 255 - s))
        out.append((np.full((8, 8), rng.integers(0, 256), np.uint8), np.full((8, 8), rng.integers(0, 256), np.uint8)))
        m = rng.integers(0, 2, (8, 8)).astype(np.uint8) * 255
        out.append((m, 255 - m))
        out.append((m, m))
        out.append((m, np.full((8, 8), 255, np.uint8)))
    return out


def test_stated_bounds_and_distance_from_real_ssim():
    """0 < a <= b < 2^29, |c| <= d < 2^28, |q1|, |q2| <= 2^20, and w / 2^20 within 2e-5 of the float64 SSIM: the header derives
    3 * 2^-20 + 0.24 / 26634 + 0.16 / 239708 < 1.3e-5."""
    worst = 0.0
    for s, r in _windows(7, 300):
        a, b, c, d, q1, q2, w = _terms(s, r)
        assert 0 < a <= b < 1 << 29 and abs(c) <= d < 1 << 28 and abs(q1) <= ONE and abs(q2) <= ONE and abs(w) <= ONE
        worst = max(worst, abs(w / ONE - cr.ssim_float(s, r)))
    assert worst < 2e-5, worst


def test_division_rounds_toward_zero():
    assert cr.cdiv(np.array([7, -7, 7, -7]), np.array([2, 2, -2, -2])).tolist() == [3, -3, -3, 3]
    # an anticorrelated window has c < 0: w is negative and rounded toward zero, not down
    m = np.indices((8, 8)).sum(0) % 2 * 255
    a, b, c, d, q1, q2, w = _terms(m.astype(np.uint8), (255 - m).astype(np.uint8))
    assert c < 0 and q2 == -((-c << 20) // d) and w == -((q1 * -q2) >> 20) and w < 0


def test_psnr_is_dump_psnrs():
    import theora_amd
    assert theora_amd.psnr(64 * 255 * 255, 64) == pytest.approx(0.0, abs=1e-12)
    assert theora_amd.psnr(100, 24 * 16) == pytest.approx(cr.psnr(100, 24 * 16))
    d = theora_amd.metrics_dict([100, 50, 50, 400, 100, 100, 3 * ONE, 0, ONE // 2, 3, 0, 1])
    assert d["ssim"] == [1.0, None, 0.5] and d["psnr"][3] == pytest.approx(cr.psnr(200, 600))


def test_kernel_body_on_the_host_stays_inside_its_rectangles(tmp_path):
    """k_picture_compare's load-and-sum body run lane by lane on the host under AddressSanitizer and UBSan
    (tests/native/picture_compare_host.cpp, a program of its own): widths and heights 1..40, offsets 0..3, the three pixel formats,
    pitches and alignments 0..15 on both sides, every byte outside the two rectangles poisoned; cell sums, squared differences and
    every window against plain loops.  The three pixel formats run side by side."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "picture_compare_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused",
           "-I" + os.path.join(root, "theora_amd", "csrc"), os.path.join(root, "tests", "native", "picture_compare_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    procs = [subprocess.Popen([exe, str(pf)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for pf in (0, 2, 3)]
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0 and out.startswith("ok: 25600 cases"), (out[-500:], err[-3000:])


def _req(**kw):
    from theora_amd import _lib
    r = _lib.PictureCompareReq()
    r.state, r.bufi, r.flags = None, -1, _lib.CMP_SSE
    r.result = 0x1000                                    # never dereferenced: every case below is refused
    for p in range(3):
        r.ref[p], r.ref_pitch[p] = 0x1000, 64
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_picture_compare_arguments_checked_without_a_state():
    from theora_amd import _lib
    L = _lib.load()
    good = _req()
    assert L.thip_picture_compare(None, 1, None) == _lib.EFAULT
    assert L.thip_picture_compare(None, 0, None) == _lib.OK
    assert L.thip_picture_compare(C.byref(good), 0, None) == _lib.OK
    assert L.thip_picture_compare(C.byref(good), -1, None) == _lib.EINVAL
    assert L.thip_picture_compare(C.byref(good), 1, None) == _lib.EFAULT       # a NULL state
    reqs = (_lib.PictureCompareReq * 10)(*([good] * 10))
    assert L.thip_picture_compare(reqs, 10, None) == _lib.EFAULT
    assert C.sizeof(_lib.PictureCompareReq) == 8 + 4 * 6 + 3 * 8 + 3 * 8 + 8 + 3 * 8 + 3 * 8      # (no padding: the header's layout)
    assert C.sizeof(_lib.PictureMetrics) == 96


def test_encoder_switch_is_checked_without_a_gpu():
    """TH_ENCCTL_THIP_SET_QUALITY_STATS never touches the GPU: the flags it takes, and the empty statistics before any packet."""
    from theora_amd import encoder
    e = encoder.Encoder(32, 32, 0, 40)
    for bad in (cr.SSIM, 4, 7, -1):
        assert e.ctl(encoder.TH_ENCCTL_THIP_SET_QUALITY_STATS, bad)[0] == -10
    for good in (cr.SSE, cr.SSE | cr.SSIM, 0):
        assert e.ctl(encoder.TH_ENCCTL_THIP_SET_QUALITY_STATS, good)[0] == 0
    q = e.quality_stats()
    assert q["measured"] == 0 and q["flags"] == 0 and q["sse"] == [0, 0, 0] and q["samples"] == [0, 0, 0]
    e.close()
