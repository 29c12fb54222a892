"""th_encode_*'s eight-mode controls without a GPU (TH_ENCCTL_THIP_SET_INTER_MODES, TH_ENCCTL_THIP_GET_MODE_STATS), and what the
restatement of the eight-mode rule (tests/enc_modes_ref.py) does on content made for it.  Nothing here reaches the first
th_encode_ycbcr_in."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_inter_ref as IR
from tests import enc_modes_ref as M
from tests import enc_ref

TH_EINVAL, TH_EIMPL = -10, -23


def _enc():
    from theora_amd import _lib
    from theora_amd.encoder import make_info
    L = _lib.load()
    info = make_info(64, 48, 0, 32)
    enc = L.th_encode_alloc(C.byref(info))
    assert enc
    return L, enc


def _ctl(L, enc, req, value, ctype=C.c_int):
    v = ctype(value)
    return L.th_encode_ctl(enc, req, C.byref(v), C.sizeof(v)), v.value


def test_mode_controls_are_known():
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_SET_INTER_MODES, E.TH_ENCCTL_THIP_GET_MODE_STATS) == (0x7209, 0x720A)
    assert E.ALL_MODE_NAMES[:5] == E.MODE_NAMES and len(E.ALL_MODE_NAMES) == 8
    assert C.sizeof(E.ModeStats) == 9 * 4
    L, enc = _enc()
    try:
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1) == (0, 1)
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_MODES, 1) == (0, 1)
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_MODES, 0) == (0, 0)
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_INTER_MODES, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_MODES, 1, C.c_int64)[0] == TH_EINVAL
        s = E.ModeStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_MODE_STATS, C.byref(s), C.sizeof(s)) == 0
        assert list(s.modes) == [0] * 8 and s.vectors == 0
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_MODE_STATS, C.byref(s), C.sizeof(s) - 4) == TH_EINVAL
    finally:
        L.th_encode_free(enc)


def test_python_encoder_all_modes():
    from theora_amd.encoder import Encoder
    e = Encoder(64, 48, 0, 20, inter=True, all_modes=True)
    assert e.all_modes and e.mode_stats() == dict(modes={n: 0 for n in e.mode_stats()["modes"]}, vectors=0)
    e.close()
    with pytest.raises(ValueError):
        Encoder(64, 48, 0, 20, all_modes=True)


def test_headers_do_not_change_with_all_modes():
    from theora_amd.encoder import Encoder
    a = Encoder(64, 48, 0, 20, inter=True, keyframe_interval=8).header_packets()
    b = Encoder(64, 48, 0, 20, inter=True, keyframe_interval=8, all_modes=True).header_packets()
    assert a == b


def test_round_div_is_the_decoders():
    for v in range(-130, 131):
        for sh in (1, 2):
            want = int(np.sign(v)) * ((abs(v) + (1 << (sh - 1))) >> sh)
            assert M.round_div(v, sh) == want, (v, sh)


def test_block_search_finds_two_motions():
    """Two 8-row bands moving apart: each luma block's own vector is its band's, and the macro blocks choose MV_FOUR."""
    rng = np.random.default_rng(4)
    ref = rng.integers(0, 256, (64, 96)).astype(np.uint8)
    pad = np.pad(ref, 8, mode="edge")
    src = np.empty_like(ref)
    for b in range(8):
        dx = 3 if b % 2 == 0 else -4
        src[8 * b:8 * b + 8] = pad[8 + 8 * b:16 + 8 * b, 8 - dx:8 - dx + 96]   # src(x, y) = ref(x - dx, y)
    ms = M.motion_search(src, ref, ref, 20)
    inner = [r * 6 + c for r in range(1, 3) for c in range(1, 5)]
    assert (ms["pix"][inner] == M.MV_FOUR).all()
    assert (ms["bmv"][inner][:, :2, 0] == -6).all() and (ms["bmv"][inner][:, 2:, 0] == 8).all()
    assert (ms["bmv"][inner][:, :, 1] == 0).all()


_CLIPS = {}


def _clip(kind, w=176, h=144, n=8, q=32):
    """(bytes, mean Y PSNR, modes8 summed) of the inter frames of the five- and eight-mode restatements, and the per-frame modes."""
    if (kind, w, h) in _CLIPS:
        return _CLIPS[(kind, w, h)]
    from theora_amd.encoder import Encoder
    setup = enc_ref.SetupParams(Encoder(w, h, 0, q).header_packets()[2])
    frames = M.sequence(kind, w, h, 0, n)
    res = {}
    for name, cls in (("five", IR.InterEncoder), ("eight", M.ModesEncoder)):
        e = cls(w, h, 0, (0, 0, w, h), setup, 64, 6)
        nbytes, ps, m8, per = 0, [], np.zeros(8, np.int64), []
        for fr in frames:
            r = e.frame(fr, q)
            per.append(r)
            if r["key"]:
                continue
            nbytes += len(r["packet"])
            err = np.mean((e.recon[0].astype(np.float64) - fr[0]) ** 2)
            ps.append(10 * np.log10(255 ** 2 / max(err, 1e-9)))
            if "modes8" in r:
                m8 += r["modes8"]
        e.close()
        res[name] = (nbytes, float(np.mean(ps)), m8, per)
    _CLIPS[(kind, w, h)] = res
    return res


def test_uncover_uses_golden_modes():
    res = _clip("uncover")
    m8 = res["eight"][2]
    assert m8[M.GOLDEN_NOMV] + m8[M.GOLDEN_MV] >= 10, m8


def test_shear_uses_four_vectors():
    res = _clip("shear")
    m8 = res["eight"][2]
    assert m8[M.MV_FOUR] >= m8.sum() // 2, m8


def test_pan_uses_neither_much():
    res = _clip("pan", 352, 288, 6)
    m8 = res["eight"][2]
    assert m8[M.GOLDEN_NOMV] + m8[M.GOLDEN_MV] + m8[M.MV_FOUR] <= m8.sum() // 20, m8


def test_no_golden_mode_right_after_a_key_frame():
    """GOLD is PREV in the frame after a key frame: CG exceeds C, so no golden mode wins there."""
    for kind in ("uncover", "shear"):
        per = _clip(kind)["eight"][3]
        assert per[0]["key"] and not per[1]["key"]
        assert per[1]["modes8"][M.GOLDEN_NOMV] == per[1]["modes8"][M.GOLDEN_MV] == 0, (kind, per[1]["modes8"])


@pytest.mark.parametrize("kind,most", [("uncover", 0.965), ("shear", 0.85)])
def test_eight_modes_take_fewer_bytes(kind, most):
    """At equal qi (32), the inter frames of 176x144 clips: measured 0.928 (uncover) and 0.694 (shear) of the five-mode bytes at
    +0.06 / +0.07 dB Y PSNR; the bounds sit at about half the gain."""
    res = _clip(kind)
    (b5, p5, _, _), (b8, p8, _, _) = res["five"], res["eight"]
    print(kind, "eight / five bytes %.3f, Y PSNR %+.3f dB" % (b8 / b5, p8 - p5))
    assert b8 <= most * b5, (b8, b5)
    assert p8 >= p5 - 0.1, (p8, p5)
