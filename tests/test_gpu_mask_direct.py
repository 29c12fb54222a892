"""thip_enc_mask_stage on the GPU: k_enc_mask_act and k_enc_mask_scale (theora_amd/csrc/thip_encode_mask.h) driven directly on the
caller's planes.  act, the average record and iscale equal tests/enc_mask_ref.py's restatement value for value, with canary bytes
around every output left untouched -- at the smallest shapes at which the kernels can go wrong: one macro block (a wave mostly
idle), an odd picture region inside the frame (the clamp on every side, rows with a pitch of their own), more luma blocks than a
work group of either kernel holds (several partials), the three pixel formats (the chroma fragment's macro block), ratios 2, 4 and
16, content that reaches the three branches of oc_mb_activity, a flat frame (A at its floor) and one noisy block in a flat frame
(the top of the range, the chroma rule)."""
import numpy as np
import pytest

from tests import enc_inter_ref as IR
from tests import enc_mask_ref as K
from tests import enc_ref
from tests.test_gpu_costmaps import _picture

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64   # bytes in front of and behind every output


def _guarded(torch, nbytes):
    t = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + GUARD


def _payload(t, nbytes, dtype):
    a = t.cpu().numpy()
    assert (a[:GUARD] == CANARY).all() and (a[GUARD + nbytes:] == CANARY).all(), "canary"
    return a[GUARD:GUARD + nbytes].view(dtype)


def _stage(hip, planes, fw, fh, fmt, pic, k, pad=13):
    """The stage on the picture region's planes (device, a pitch that is neither the width nor a multiple of 4): act, rec, iscale."""
    import torch
    from theora_amd import encoder as E
    geo = IR.Geometry(fw, fh, fmt)
    nluma = geo.planes[0]["nfrags"]
    dev = []
    for p in range(3):
        x0, y0, cw, ch = enc_ref.chroma_region(pic, fmt, p)
        a = np.asarray(planes[p])
        if a.shape != (ch, cw):
            a = a[y0:y0 + ch, x0:x0 + cw]
        t = torch.full((ch, cw + pad), 77, dtype=torch.uint8, device="cuda")
        t[:, :cw] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dev.append(t)
    act, pa = _guarded(torch, nluma * 4)
    rec, pr = _guarded(torch, 16)
    isc, pi = _guarded(torch, geo.nfrags * 2)
    rc = E.mask_stage((fw, fh), fmt, k, pic=pic, src=[t.data_ptr() for t in dev], src_pitch=[t.stride(0) for t in dev], act=pa, avg=pr,
                      iscale=pi)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return geo, _payload(act, nluma * 4, np.uint32), _payload(rec, 16, np.uint64), _payload(isc, geo.nfrags * 2, np.uint16)


def _check(hip, planes, fw, fh, fmt, pic, k):
    geo, act, rec, isc = _stage(hip, planes, fw, fh, fmt, pic, k)
    want_act = K.activity(planes, fw, fh, fmt, pic)
    assert np.array_equal(act.astype(np.int64), want_act), np.argwhere(act != want_act)[:4].tolist()
    want_isc, A, amax = K.scales(want_act, k, geo)
    assert rec.tolist() == [A, amax], (rec.tolist(), A, amax)
    assert np.array_equal(isc.astype(np.int64), want_isc), np.argwhere(isc != want_isc)[:4].tolist()
    assert isc.min() >= 2048 // k and isc.max() <= 2048 * k
    return geo, want_act, want_isc, A


SHAPES = [   # (frame, pixel format, picture region, ratio)
    (16, 16, 0, None, 4),
    (16, 16, 3, None, 2),
    (32, 32, 2, None, 16),
    (64, 48, 0, None, 4),
    (64, 48, 2, None, 2),
    (64, 48, 3, None, 16),
    (80, 64, 0, (5, 3, 67, 49), 4),
    (80, 64, 2, (5, 3, 67, 49), 16),
    (80, 64, 3, (5, 3, 67, 49), 2),
    (80, 64, 0, (0, 0, 9, 9), 4),      # a picture narrower than the twelve bytes the fast rows read
    (352, 288, 0, None, 4),            # 1584 luma blocks: seven partials; 2376 fragments: ten work groups of the scale kernel
    (352, 288, 3, (3, 1, 345, 280), 2),
]


@pytest.mark.parametrize("fw,fh,fmt,pic,k", SHAPES)
def test_stage_equals_the_restatement(hip, fw, fh, fmt, pic, k):
    rng = np.random.default_rng(fw + 3 * fh + fmt + k)
    planes = _picture(rng, fw, fh, fmt)
    pic = pic or (0, 0, fw, fh)
    geo, act, isc, A = _check(hip, planes, fw, fh, fmt, pic, k)
    if fw * fh >= 64 * 48 and pic[2] > 16:   # the three branches of oc_mb_activity: flat, texture, damped edge
        assert (act <= 5 << 12).any() and (act >= 8 << 12).any()


@pytest.mark.parametrize("fw,fh,fmt", [(64, 48, 0), (176, 144, 3), (352, 288, 2)])
def test_whole_frame_activity_is_the_cost_maps(hip, fw, fh, fmt):
    """Where the picture region is the whole frame, act is thip_enc_mb_cost_maps' activity of the input, value for value."""
    import torch
    rng = np.random.default_rng(fw + fmt)
    planes = _picture(rng, fw, fh, fmt)
    geo, act, rec, isc = _stage(hip, planes, fw, fh, fmt, (0, 0, fw, fh), 4)
    dev = [torch.from_numpy(np.ascontiguousarray(np.flipud(p))).cuda() for p in planes]   # (bitstream row order)
    maps = hip.enc_mb_cost_maps(dev, fw, fh, fmt)[2].cpu().numpy().view(np.uint32)
    assert np.array_equal(K.luma_raster(maps, fw, fh).reshape(-1), act)


@pytest.mark.parametrize("k", [2, 4, 16])
def test_a_flat_frame(hip, k):
    """Every activity 0: A at its floor of 64, every luma scale 2048 / k, every chroma scale 2048."""
    fw, fh = 64, 48
    planes = [np.full((fh, fw), 93, np.uint8), np.full((fh // 2, fw // 2), 10, np.uint8), np.full((fh // 2, fw // 2), 200, np.uint8)]
    geo, act, rec, isc = _stage(hip, planes, fw, fh, 0, (0, 0, fw, fh), k)
    assert not act.any() and rec.tolist() == [64, 0]
    nl = geo.planes[0]["nfrags"]
    assert (isc[:nl] == 2048 // k).all() and (isc[nl:] == 2048).all()
    _check(hip, planes, fw, fh, 0, (0, 0, fw, fh), k)


@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_one_noisy_block_in_a_flat_frame(hip, fmt):
    """The block sits high in the range, the flat ones at its bottom; its macro block's chroma takes the second least luma scale,
    floored (one noisy block: 2048), and with all four blocks noisy the least of them."""
    fw, fh, k = 64, 48, 4
    rng = np.random.default_rng(9)
    cw, ch = fw >> int(not fmt & 1), fh >> int(not fmt & 2)
    planes = [np.full((fh, fw), 120, np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)]
    planes[0][16:24, 32:40] = rng.integers(0, 256, (8, 8))          # one block of macro block (2, 1) from the top
    planes[0][32:48, 0:16] = rng.integers(0, 256, (16, 16))         # all four of macro block (0, 2)
    geo, act, isc, A = _check(hip, planes, fw, fh, fmt, (0, 0, fw, fh), k)
    nh = fw >> 3
    by, bx = (fh >> 3) - 1 - 2, 4                                   # the noisy block, rows from the bottom
    nl = nh * (fh >> 3)
    assert isc[by * nh + bx] > 2 * 2048 and act[by * nh + bx] > 8 << 12
    flat = np.ones(nl, bool)
    flat[[by * nh + bx, 0, 1, nh, nh + 1]] = False
    assert not act[flat].any() and (isc[:nl][flat] == 2048 // k).all()   # activity 0: the bottom of the range
    mb_noisy1, mb_noisy4 = (by >> 1) * geo.nmbx + (bx >> 1), 0
    for p in (1, 2):
        g = geo.planes[p]
        fi = g["froffset"] + np.arange(g["nfrags"])
        one, four = isc[fi[geo.mb_of[fi] == mb_noisy1]], isc[fi[geo.mb_of[fi] == mb_noisy4]]
        assert one.size == four.size == (1 if fmt == 0 else 2 if fmt == 2 else 4)
        assert (one == 2048).all()                                   # three flat blocks: the second least lies under 2048
        assert (four == isc[[0, 1, nh, nh + 1]].min()).all() and four.min() > 2048
        rest = isc[fi[(geo.mb_of[fi] != mb_noisy1) & (geo.mb_of[fi] != mb_noisy4)]]
        assert (rest == 2048).all()
