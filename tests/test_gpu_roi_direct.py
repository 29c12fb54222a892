"""thip_enc_roi_stage on the GPU: k_enc_roi_scale and k_enc_roi_fold (theora_amd/csrc/thip_encode_roi.h) driven directly on the
caller's map.  Every iscale and every statistics word equals tests/enc_roi_ref.roi_scales, with canary bytes around both outputs left
untouched -- at the smallest shapes at which the kernel can go wrong: the three pixel formats, an odd picture region inside the frame
(the clamp on every side), a fragment count that is no multiple of the work group (496 x 496), map widths and heights at, one below
and one above every switch between the kernel's three ways to a block's sum (a block's columns meet a third cell between pw / 16 and
pw / 4 map columns; they span eight cells from about pw / 2 for a decimated plane and pw for luma), a map finer than pixels, bases and
pitches that are no multiple of 4 and negative pitches (the dword path needs both aligned), with and without masking's scales in, in
place and not; and one 3840 x 2160 case, scales only."""
import numpy as np
import pytest

from tests import enc_inter_ref as IR
from tests import enc_roi_ref as R

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


def _device_map(torch, v, pad, off, neg):
    """v [hm][wm] on the device at pitch wm + pad (negative: row 0 last in memory), row 0 `off` bytes past a 256-byte boundary;
    every byte that is no entry holds 127, which no map holds.  Returns (the tensor, row 0's address, the pitch)."""
    hm, wm = v.shape
    ap = wm + pad
    host = np.full(off + hm * ap + 8, 127, np.int8)
    rows = host[off:off + hm * ap].reshape(hm, ap)
    rows[:, :wm] = v[::-1] if neg else v
    t = torch.from_numpy(host).cuda()
    base = t.data_ptr() + off
    return t, (base + (hm - 1) * ap, -ap) if neg else (base, ap)


def _stage(geo, fw, fh, fmt, pic, v, mask=None, pad=0, off=0, neg=False, in_place=False):
    import torch
    from theora_amd import encoder as E
    t, (ptr, pitch) = _device_map(torch, v, pad, off, neg)
    isc, pi = _guarded(torch, geo.nfrags * 2)
    st, ps = _guarded(torch, 32)
    pm = keep = None
    if mask is not None:
        m16 = torch.from_numpy(np.asarray(mask).astype(np.uint16).view(np.int16)).cuda()
        if in_place:
            isc[GUARD:GUARD + geo.nfrags * 2] = m16.view(torch.uint8)
            pm = pi
        else:
            keep, pm = m16, m16.data_ptr()
    rc = E.roi_stage((fw, fh), fmt, (v.shape[1], v.shape[0]), pitch, ptr, pic=pic, mask_iscale=pm, iscale=pi, stats=ps)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return _payload(isc, geo.nfrags * 2, np.uint16), _payload(st, 32, np.int32)


def _check(geo, fw, fh, fmt, pic, v, mask=None, **kw):
    isc, st = _stage(geo, fw, fh, fmt, pic, v, mask, **kw)
    want, ws = R.roi_scales(geo, pic, fmt, v, mask)
    assert np.array_equal(isc.astype(np.int64), want), ((v.shape, kw), np.argwhere(isc != want)[:4].tolist())
    assert st.tolist() == [ws["exp_min"], ws["exp_max"], ws["exp_sum"] & 0xFFFFFFFF if ws["exp_sum"] >= 0 else ws["exp_sum"],
                           0 if ws["exp_sum"] >= 0 else -1, ws["scale_min"], ws["scale_max"], 0, 0], (v.shape, kw, st.tolist(), ws)


def _sizes(n):
    """Map sizes along a picture side of n pixels: at, below and above every switch."""
    s = {1, 2, 3, n // 16, n // 16 + 1, n // 8 - 1, n // 8, n // 8 + 1, n // 4, n // 4 + 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n, n + 1,
         2 * n - 1, 2 * n, 2 * n + 1, 3 * n + 5}
    return sorted(k for k in s if k >= 1)


GEOS = [(64, 48, (0, 0, 64, 48)), (80, 64, (5, 3, 67, 49)), (496, 496, (0, 0, 496, 496))]


@pytest.mark.parametrize("fmt", [0, 2, 3])
@pytest.mark.parametrize("fw,fh,pic", GEOS)
def test_stage_equals_the_restatement_round_every_switch(hip, fw, fh, pic, fmt):
    geo = IR.Geometry(fw, fh, fmt)
    rng = np.random.default_rng(fw + fmt)
    ws, hs = _sizes(pic[2]), _sizes(pic[3])
    if fw > 80:   # (the large frame: the switches along the width, three heights)
        hs = [pic[3] // 16, pic[3] // 2 + 1, pic[3] + 1]
    n = 0
    for wm in ws:
        for hm in (hs if fw > 80 else hs[n % 3::3]):   # (a third of the heights a width, every height with some width)
            v = rng.integers(-64, 65, (hm, wm)).astype(np.int8)
            mask = rng.integers(128, 32769, geo.nfrags) if n % 2 else None
            _check(geo, fw, fh, fmt, pic, v, mask, pad=(0, 1, 4, 7)[n % 4], off=(0, 0, 1, 3)[(n // 4) % 4], neg=n % 5 == 4,
                   in_place=n % 4 == 3)
            n += 1


@pytest.mark.parametrize("pad,off,neg", [(0, 0, False), (4, 0, True), (0, 1, False), (1, 0, False), (3, 2, True), (8, 0, False)])
def test_aligned_and_misaligned_maps_agree(hip, pad, off, neg):
    """One map at pixel resolution (the dword path where the base and the pitch are multiples of 4, bytes elsewhere) and one at the
    macro-block grid, at every kind of base and pitch: the same scales."""
    fw, fh, pic = 80, 64, (5, 3, 67, 49)
    rng = np.random.default_rng(7)
    for fmt in (0, 3):
        geo = IR.Geometry(fw, fh, fmt)
        for wm, hm in ((67, 49), (68, 49), (64, 12), (5, 4)):
            v = rng.integers(-64, 65, (hm, wm)).astype(np.int8)
            _check(geo, fw, fh, fmt, pic, v, None, pad=pad, off=off, neg=neg)


def test_the_ends_of_the_range(hip):
    """Uniform maps at both ends with masking's scales at both ends: the exponent's ends, both clamps of the final scale."""
    fw, fh, pic = 64, 48, (0, 0, 64, 48)
    geo = IR.Geometry(fw, fh, 0)
    mask = np.full(geo.nfrags, 2048, np.int64)
    mask[::2], mask[1::3] = 128, 32768
    for v in (-64, -63, -17, -16, -1, 0, 1, 15, 16, 63, 64):
        _check(geo, fw, fh, 0, pic, np.full((2, 2), v, np.int8), mask)
        _check(geo, fw, fh, 0, pic, np.full((1, 1), v, np.int8))


def test_the_longest_maps(hip):
    fw, fh, pic = 80, 64, (5, 3, 67, 49)
    geo = IR.Geometry(fw, fh, 0)
    rng = np.random.default_rng(3)
    for wm, hm in ((16384, 1), (1, 16384), (16384, 3)):
        _check(geo, fw, fh, 0, pic, rng.integers(-64, 65, (hm, wm)).astype(np.int8), pad=1 if wm == 1 else 0)


@pytest.mark.parametrize("wm,hm", [(240, 135), (3840, 2160)], ids=["macro-blocks", "pixels"])
def test_a_4k_frame(hip, wm, hm):
    """3840 x 2160 4:2:0 in a 3840 x 2176 frame: 195840 fragments, 765 work groups, scales only."""
    fw, fh, pic = 3840, 2176, (0, 0, 3840, 2160)
    geo = IR.Geometry(fw, fh, 0)
    rng = np.random.default_rng(wm)
    v = rng.integers(-64, 65, (hm, wm)).astype(np.int8)
    isc, st = _stage(geo, fw, fh, 0, pic, v)
    want = R.roi_scales(geo, pic, 0, v)[0]
    assert np.array_equal(isc.astype(np.int64), want)
