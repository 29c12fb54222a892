"""The device paths against the reference codec itself (oracle/ref.py; oracle/_ref/libtheora_ref.so travels with the working tree,
the reference's source tree is never read here).  Everything is integer and exact.

Decode: streams the reference encoder makes on this machine's CPU, through th_decode_* on the device in the default configuration
and in every alternative with kernels or a hand-over of its own; every plane of every frame equals the reference decoder's.
Encode: the packets of th_encode_*, feature by feature, through the reference decoder: none refused, the same granule positions,
the pictures our own th_decode_* makes from them, and the encoder's own reconstruction.  The batched block kernels and the
post-processing filters against the reference's functions directly."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import ref
from tests import enc_ref, refcmp, util

pytestmark = pytest.mark.gpu
CPU_SECONDS = dict(reference=0.0)      # time spent inside the reference on the CPU, for the log


@pytest.fixture(scope="module", autouse=True)
def _tally():
    t0 = time.time()
    yield
    print("\nreference comparisons of this module: %d frames, %d planes; %.1f s in all, %.1f s of them in the reference encoder and "
          "decoder on the CPU" % (refcmp.TALLY["frames"], refcmp.TALLY["planes"], time.time() - t0, CPU_SECONDS["reference"]))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- decode -------------------------------------------------------------------------------------------------------------------------
STREAMS = {   # name: (w, h, fmt, pic, content, frames, reference encoder arguments)
    "qcif_q32": (176, 144, 0, None, "lcg", 24, dict(quality=32, kf_interval=64)),
    "qcif_q0": (176, 144, 0, None, "natural", 20, dict(quality=0, kf_interval=64)),
    "qcif_q63": (176, 144, 0, None, "natural", 20, dict(quality=63, kf_interval=64)),
    "qcif_bitrate": (176, 144, 0, None, "natural", 24, dict(quality=0, bitrate=120000, kf_interval=64)),
    "422": (80, 48, 2, None, "natural", 20, dict(quality=32, kf_interval=64)),
    "444": (48, 64, 3, None, "natural", 20, dict(quality=32, kf_interval=64)),
    "odd_region": (80, 64, 0, (3, 5, 61, 43), "natural", 20, dict(quality=32, kf_interval=64)),
    "720p": (1280, 720, 0, None, "lcg", 20, dict(quality=32, kf_interval=64)),
    "1080p": (1920, 1088, 0, (0, 4, 1920, 1080), "lcg_t", 3, dict(quality=32, kf_interval=64)),
}
_MADE = {}


def _stream(name):
    """(headers, packets, granule positions, the reference decoder's pictures), made once a session."""
    if name not in _MADE:
        refcmp.need_ref()
        w, h, fmt, pic, kind, n, kw = STREAMS[name]
        frames = refcmp.lcg_frames(w, h, fmt, n, temporal=kind == "lcg_t") if kind.startswith("lcg") else refcmp.moving(kind, w, h, fmt, n, 3)
        t0 = time.time()
        hdr, pk = refcmp.ref_encode(frames, w, h, fmt, pic=pic, **kw)
        rd = ref.RefDecoder(hdr)
        pics = []
        for p, gp in pk:
            assert rd.packetin(p) == (0 if p else 1, gp)
            pics.append(rd.ycbcr_out())
        rd.close()
        CPU_SECONDS["reference"] += time.time() - t0
        assert len(pk) == n and any(p and p[0] & 0x40 for p, _ in pk)      # inter frames among them
        _MADE[name] = (hdr, [p for p, _ in pk], [g for _, g in pk], pics)
    return _MADE[name]


LISTS, TOKENS, DC = "TH_DECCTL_THIP_SET_DEVICE_LISTS", "TH_DECCTL_THIP_SET_DEVICE_TOKENS", "TH_DECCTL_THIP_SET_DEVICE_DC"
VARIANTS = {   # name: (library options, th_decode_ctl requests (name in theora_amd.decoder, value), packets announced ahead)
    "default": ({}, [], 0),
    "two_passes": (dict(fuse=0), [], 0),
    "host_walk": ({}, [(LISTS, 0)], 0),                        # the host's own token walk
    "device_tokens": ({}, [(LISTS, 0), (TOKENS, 1)], 0),
    "device_dc": ({}, [(LISTS, 0), (DC, 1)], 0),
    "device_tokens_dc": ({}, [(LISTS, 0), (TOKENS, 1), (DC, 1)], 0),
    "device_lists_announced": ({}, [(LISTS, 1)], 3),           # TH_DECCTL_THIP_PREFETCH_PACKET, three ahead
    "host_walk_announced": ({}, [(LISTS, 0)], 2),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(STREAMS))
def test_reference_encoded_streams_decode_on_the_device(hip, name, variant):
    from theora_amd import _lib, decoder
    from theora_amd.decoder import Decoder
    hdr, packets, gps, pics = _stream(name)
    opts, ctls, ahead = VARIANTS[variant]
    with util.options(_lib.load(), **opts):
        dec = Decoder(hdr)
        for code, value in ctls:
            v = C.c_int(value)
            assert dec._L.th_decode_ctl(dec._dec, getattr(decoder, code), C.byref(v), C.sizeof(v)) == 0, code
        announced = taken = 0
        for f, pkt in enumerate(packets):
            while ahead and announced < len(packets) and announced < f + ahead:
                announced = max(announced, f)
                if dec.prefetch(packets[announced]):
                    taken += 1
                elif len(packets[announced]):
                    break
                announced += 1
            rc, gp = dec.packetin(pkt)
            assert (rc, gp) == (0 if pkt else 1, gps[f]), f
            bad = refcmp.diff_planes(dec.ycbcr_out(), pics[f])
            assert not bad, (f, bad)
            refcmp.TALLY["frames"] += 1
        dec.close()
    if ahead:
        assert taken >= len(packets) - 2, taken


def test_cropped_picture_out_equals_the_references_picture_region(hip):
    """TH_DECCTL_THIP_PICTURE_OUT, planar Y'CbCr of the cropped picture, for the stream with an odd picture region."""
    from theora_amd.decoder import Decoder
    hdr, packets, gps, pics = _stream("odd_region")
    w, h, fmt, pic = STREAMS["odd_region"][:4]
    dec = Decoder(hdr)
    for f, pkt in enumerate(packets):
        dec.packetin(pkt)
        got = [t.cpu().numpy() for t in dec.picture(fmt="ycbcr", crop=True)]
        want = []
        for p in range(3):
            x0, y0, cw, ch = enc_ref.chroma_region(pic, fmt, p)
            want.append(pics[f][p][y0:y0 + ch, x0:x0 + cw])
        assert got[0].shape == (pic[3], pic[2])
        bad = refcmp.diff_planes(got, want)
        assert not bad, (f, bad)
    dec.close()


def test_fixture_decodes_on_the_device(hip):
    """tests/golden/ref_qcif_q32.npz (made by the reference encoder, digests by the reference decoder) through th_decode_*: needs no
    oracle/_ref/."""
    from theora_amd.decoder import Decoder
    hdr, packets, gps, digests = refcmp.load_fixture()
    dec = Decoder(hdr)
    for f, pkt in enumerate(packets):
        assert dec.packetin(pkt) == (0, gps[f])
        assert refcmp.digest(dec.ycbcr_out()) == digests[f], f
    dec.close()


# ---- encode -------------------------------------------------------------------------------------------------------------------------
FEATURES = {   # name: (Encoder arguments, content)
    "intra": (dict(), "pan"),
    "five_modes": (dict(inter=True, keyframe_interval=5), "pan"),
    "eight_modes": (dict(inter=True, keyframe_interval=5, all_modes=True), "shear"),
    "eight_modes_uncover": (dict(inter=True, keyframe_interval=5, all_modes=True), "uncover"),
    "block_qi_4": (dict(inter=True, keyframe_interval=5, all_modes=True, block_qi=4), "shear"),
    "block_qi_9": (dict(inter=True, keyframe_interval=5, block_qi=9), "pan"),
    "bitrate": (dict(inter=True, keyframe_interval=5, bitrate=15000), "cut"),
}
GEOMETRIES = [(176, 144, 0, None), (96, 64, 0, None), (64, 48, 2, (1, 2, 61, 45)), (48, 64, 3, None), (16, 16, 0, None)]
NFRAMES = 12     # more than two key-frame intervals of 5: the golden frame is refreshed twice


def _cropped(frames, fmt, pic):
    if pic is None:
        return frames
    reg = [enc_ref.chroma_region(pic, fmt, p) for p in range(3)]
    return [[np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in zip(fr, reg)] for fr in frames]


@pytest.mark.parametrize("pack", [False, True], ids=["host_pack", "device_pack"])
@pytest.mark.parametrize("w,h,fmt,pic", GEOMETRIES, ids=["qcif", "96x64", "422_odd_region", "444", "one_macro_block"])
@pytest.mark.parametrize("feature", list(FEATURES))
def test_encoder_packets_decode_in_the_reference(hip, feature, w, h, fmt, pic, pack):
    """th_encode_*'s packets through the reference decoder: none is refused; its granule positions are th_encode_packetout's; its
    pictures are the ones our own th_decode_* makes from the same packets, and the encoder's reconstruction where it hands one out
    (inter frames on)."""
    from tests import enc_modes_ref as M
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import ALL_MODE_NAMES, Encoder
    refcmp.need_ref()
    kw, kind = FEATURES[feature]
    frames = _cropped(M.sequence(kind, w, h, fmt, NFRAMES, seed=5), fmt, pic)
    e = Encoder(w, h, fmt, 32, pic=pic, device_pack=pack, **kw)
    hdr = e.header_packets()
    rd, dec = ref.RefDecoder(hdr), Decoder(hdr)
    info = rd.info.as_dict()
    assert (info["frame_width"], info["frame_height"], info["pixel_fmt"]) == (w, h, fmt)
    dropped = keys = 0
    modes, qii_used, several_qi = np.zeros(8, np.int64), set(), []
    for f, fr in enumerate(frames):
        e.encode(fr)
        pkt, gp, _, _ = e.packetout(f == NFRAMES - 1)
        assert e.packetout(f == NFRAMES - 1) is None
        if "bitrate" in kw:
            dropped += int(e.rate_stats()["dropped"])
        if pack and pkt:
            assert e.pack_stats()["device"] == 1, f          # (the packet did come from the device packetiser)
        t0 = time.time()
        rc, rgp = rd.packetin(pkt)
        want = rd.ycbcr_out()
        CPU_SECONDS["reference"] += time.time() - t0
        assert rc == (0 if pkt else 1), (f, rc)
        assert rgp == gp, (f, rgp, gp)
        keys += int(bool(pkt) and not pkt[0] & 0x40)
        if pkt and pkt[0] & 0x40 and kw.get("all_modes"):
            modes += [e.mode_stats()["modes"][k] for k in ALL_MODE_NAMES]
        if pkt and kw.get("block_qi"):
            several_qi.append(refcmp.more_than_one_qi(pkt))
            qii_used |= {k for k, row in enumerate(e.block_qi_stats()["blocks"]) if sum(row)}
        assert dec.packetin(pkt) == (rc, gp)
        bad = refcmp.diff_planes(dec.ycbcr_out(), want)
        assert not bad, (f, "th_decode_*", bad)
        if kw.get("inter"):
            bad = refcmp.diff_planes(e.recon(), want)
            assert not bad, (f, "encoder's reconstruction", bad)
        refcmp.TALLY["frames"] += 1
    e.close()
    rd.close()
    dec.close()
    assert keys >= (3 if kw.get("inter") else NFRAMES) or "bitrate" in kw
    # the feature the case is named after is in the packets the reference decoded
    print(feature, (w, h, fmt), "modes", modes.tolist(), "qii used", sorted(qii_used), "packets with several qi", sum(several_qi))
    if kw.get("block_qi"):
        assert several_qi and all(several_qi)                     # every coded frame lists more than one qi
        assert len(qii_used) >= 2 or w < 176                      # and on the QCIF content the blocks do not all take the same one
    if feature == "eight_modes_uncover" and w == 176:
        assert modes[5] + modes[6] > 0                            # golden-frame modes
    if feature == "eight_modes" and w == 176:
        assert modes[7] > 0                                       # four vectors a macro block
    if feature == "bitrate" and (w, h) == (96, 64):
        assert dropped >= 1           # a dropped frame went through both decoders


# ---- the batched kernels against the reference's functions ---------------------------------------------------------------------------
def test_idct_batch_equals_the_reference(hip):
    refcmp.need_ref()
    for seed in (0, 1):
        x, lz = refcmp.idct_inputs(seed)
        got = hip.idct8x8_batch(dev(x), dev(lz)).cpu().numpy()
        want = ref.idct8x8(x, lz)
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert bad.size == 0, (seed, bad[:5], lz[bad[:5]])
    assert set(lz.tolist()) == set(range(65))


def test_fdct_batch_equals_the_reference(hip):
    refcmp.need_ref()
    for seed in (0, 1):
        x = refcmp.fdct_inputs(seed)
        assert np.array_equal(hip.fdct8x8_batch(dev(x)).cpu().numpy(), ref.fdct8x8(x)), seed


@pytest.mark.parametrize("lanes", [4, 1])
def test_fdct_quantise_batch_equals_the_reference(hip, lanes):
    """thip_enc_fdct_quantize_batch (both kernels, option enc_fq_lanes) == oc_enc_fdct8x8_c then oc_enc_quantize_c, and
    thip_enc_quantize_batch == oc_enc_quantize_c on coefficients at the rounding thresholds, for tables of our own setup header."""
    from theora_amd import _lib
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    e = Encoder(64, 48, 0, 32)
    setup = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    rng = np.random.default_rng(13)
    x = refcmp.fdct_inputs(2)
    with util.options(_lib.load(), enc_fq_lanes=lanes):
        for qi, qti, pli in ((0, 0, 0), (0, 1, 1), (20, 0, 2), (32, 1, 0), (47, 0, 0), (63, 0, 0), (63, 1, 2)):
            dq = setup.qmat(qti, pli, qi)[refcmp.ZIGZAG].astype(np.uint16)
            dct = ref.fdct8x8(x)
            want, wnz = ref.quantize(dct, dq)
            q, nz, gd = hip.enc_fdct_quantize_batch(dev(x), dev(dq), want_dct=True)
            assert np.array_equal(gd.cpu().numpy(), dct), (qi, qti, pli)
            assert np.array_equal(q.cpu().numpy(), want) and np.array_equal(nz.cpu().numpy(), wnz), (qi, qti, pli)
            edge = refcmp.quant_inputs(dq, rng)
            want, wnz = ref.quantize(edge, dq)
            q, nz = hip.enc_quantize_batch(dev(edge), dev(dq))
            assert np.array_equal(q.cpu().numpy(), want) and np.array_equal(nz.cpu().numpy(), wnz), (qi, qti, pli)


@pytest.mark.parametrize("op", ["sad", "sad_thresh", "sad2_thresh", "intra_sad", "satd", "satd2", "intra_satd", "ssd"])
def test_metric_batch_equals_the_reference(hip, op):
    refcmp.need_ref()
    for seed in (0, 1):
        src, rf = refcmp.pixel_planes(seed)
        h, w = src.shape
        so, ro, r2 = refcmp.block_offsets(seed, w, h, 400)
        plain, _ = ref.metric("sad2_thresh" if op == "sad2_thresh" else "sad", src, rf, w, so, ro, r2, 0xFFFFFFFF)
        med, top = int(np.median(plain)), int(plain.max())
        for th in ([0, 1, med - 1, med, med + 1, top, top + 1, 1 << 30] if "thresh" in op else [0]):
            want, wdc = ref.metric(op, src, rf, w, so, ro, r2, th)
            got, gdc = hip.enc_metric_batch(op, dev(src), dev(rf), w, dev(so), dev(ro), dev(r2), th)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (seed, th)
            if "satd" in op:
                assert np.array_equal(gdc.cpu().numpy(), wdc), (seed, th)


# ---- post-processing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("name", ["qcif_q0", "720p"])
def test_postprocessing_on_the_device_equals_the_reference(hip, name, level):
    """TH_DECCTL_SET_PPLEVEL through th_decode_* (thip_state_postprocess: k_pp_hedge, k_pp_vedge, k_pp_dering) against the reference
    decoder at the same level, on reference-encoded streams."""
    from theora_amd.decoder import Decoder
    hdr, packets, gps, plain = _stream(name)
    packets = packets[:8 if name == "qcif_q0" else 3]
    t0 = time.time()
    rd = ref.RefDecoder(hdr)
    rd.set_pp_level(level)
    want = []
    for p in packets:
        rd.packetin(p)
        want.append(rd.ycbcr_out())
    rd.close()
    CPU_SECONDS["reference"] += time.time() - t0
    dec = Decoder(hdr)
    lv = C.c_int(level)
    assert dec._L.th_decode_ctl(dec._dec, ref.TH_DECCTL_SET_PPLEVEL, C.byref(lv), C.sizeof(lv)) == 0
    changed = 0
    for f, p in enumerate(packets):
        dec.packetin(p)
        bad = refcmp.diff_planes(dec.ycbcr_out(), want[f])
        assert not bad, (f, bad)
        changed += sum(int((a != b).sum()) for a, b in zip(want[f], plain[f]))
        refcmp.TALLY["frames"] += 1
    dec.close()
    assert (changed > 0) == (level >= 2)
