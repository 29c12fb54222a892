"""The oracle, the decoder front end and the encoder's stated rules against the reference codec itself (oracle/ref.py: the
reference's own C sources built into oracle/_ref/libtheora_ref.so), without a GPU.  Everything is integer and exact.

What is compared: the block kernels of oracle/theora_oracle.c with the reference's functions of the same name; whole streams
(tests/streamgen.py's, and streams the reference encoder makes) through the reference decoder, through oracle.State, and through
theora_amd.decoder.Decoder in slot-trace mode; our encoder's header packets through the reference's th_decode_headerin; the
packets of the encoder restatements (tests/enc_*_ref.py) through the reference decoder; the oracle's post-processing.

Where neither oracle/_ref/ nor the reference tree exists the tests that need the library skip; the fixture tests at the end of the
file run everywhere.

No input is excluded: nothing met so far has undefined behaviour in the reference or differs between its C and SIMD paths.  An
input that does is to be named here and left out by name, never as a share of randomly drawn ones."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from oracle import ref
from tests import enc_ref, refcmp, streamgen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _tally():
    yield
    print("\nreference comparisons of this module: %(frames)d frames, %(planes)d planes, %(blocks)d blocks" % refcmp.TALLY)


# ---- the recipe ---------------------------------------------------------------------------------------------------------------------
def test_two_libraries_one_process():
    """libtheora_ref.so and libtheora_hip.so export th_decode_* under the same names and live in one process: each decodes the same
    stream through its own code (different version strings, the same picture), and a request only ours knows is refused by the
    reference's handle and honoured by ours."""
    from theora_amd import _lib
    from theora_amd.decoder import Decoder, SlotTrace, TH_DECCTL_THIP_GET_SLOT_TRACE
    RL = refcmp.need_ref()
    L = _lib.load()
    assert b"Xiph" in RL.th_version_string() and b"Xiph" not in L.th_version_string()
    for name in ("th_decode_packetin", "th_encode_ycbcr_in", "th_info_init"):
        assert C.cast(getattr(RL, name), C.c_void_p).value != C.cast(getattr(L, name), C.c_void_p).value, name
    st = streamgen.Stream(32, 32, 0, seed=11)
    hdr = st.header_packets()
    pkt, truth = st.frame(0)
    bad, _ = refcmp.compare_stream(hdr, [pkt], 32, 32, 0)
    assert not bad, bad
    rd = ref.RefDecoder(hdr)
    with refcmp.trace_mode():
        dec = Decoder(hdr)
        assert rd.packetin(pkt) == dec.packetin(pkt)
        t = SlotTrace()
        assert rd.ctl(TH_DECCTL_THIP_GET_SLOT_TRACE, C.byref(t), C.sizeof(t)) == ref.TH_EIMPL
        assert L.th_decode_ctl(dec._dec, TH_DECCTL_THIP_GET_SLOT_TRACE, C.byref(t), C.sizeof(t)) == 0
        assert t.ncoded == int(truth["coded"].sum())
        dec.close()
    rd.close()


def test_the_recipe_names_sources_and_nothing_more():
    """oracle/ref.py builds from the reference tree's own files; the shim under oracle/ref_shim/ is ours and small."""
    shim = os.path.join(os.path.dirname(ref.__file__), "ref_shim")
    assert sorted(os.listdir(shim)) == ["bitwriter.c", "ogg"] and os.listdir(os.path.join(shim, "ogg")) == ["ogg.h"]
    assert os.path.getsize(os.path.join(shim, "bitwriter.c")) < 4096 and os.path.getsize(os.path.join(shim, "ogg", "ogg.h")) < 4096
    assert len(ref.DEC_UNITS) == 13 and len(ref.ENC_UNITS) == 12


# ---- block kernels: the oracle's function against the reference's -----------------------------------------------------------------
def _golden():
    return np.load(os.path.join(GOLDEN, "kernels.npz"))


def test_idct_equals_the_reference():
    refcmp.need_ref()
    g = _golden()
    assert np.array_equal(ref.idct8x8(g["idct_x"], g["idct_last_zzi"]), g["idct_y"])
    for seed in (0, 1):
        x, lz = refcmp.idct_inputs(seed)
        want = ref.idct8x8(x, lz)
        got = oracle.idct8x8_batch(x, lz)
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert bad.size == 0, (seed, bad[:5], lz[bad[:5]])
        refcmp.TALLY["blocks"] += len(x)
    assert set(lz.tolist()) == set(range(65))


def test_fdct_equals_the_reference():
    refcmp.need_ref()
    g = _golden()
    assert np.array_equal(ref.fdct8x8(g["fdct_x"]), g["fdct_y"])
    for seed in (0, 1):
        x = refcmp.fdct_inputs(seed)
        assert np.array_equal(ref.fdct8x8(x), oracle.fdct8x8_batch(x)), seed
        refcmp.TALLY["blocks"] += len(x)


def _residues(rng, n):
    """Residue blocks that clamp at both ends, barely and not at all."""
    r = [rng.integers(-300, 301, 64) for _ in range(n)] + [rng.integers(-5, 6, 64) for _ in range(n)]
    r += [np.full(64, v) for v in (-32768, 32767, -256, -255, -129, -128, -127, 0, 126, 127, 128, 255, 256)]
    return np.array(r, np.int16)


def test_recon_and_copy_equal_the_reference():
    RL = refcmp.need_ref()
    OL = oracle.lib()
    OL.orc_frag_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    rng = np.random.default_rng(3)
    stride = 24
    res = _residues(rng, 60)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)   # noqa: E731
    for k, r in enumerate(res):
        s1 = rng.integers(0, 256, (10, stride)).astype(np.uint8)
        s2 = rng.integers(0, 256, (10, stride)).astype(np.uint8)
        if k % 5 == 0:
            s1[:] = 255 * (k & 1)
            s2[:] = 255 * (k >> 1 & 1)
        off = int(rng.integers(0, 2)) * stride + int(rng.integers(0, stride - 8))
        outs = []
        for which in (0, 1):
            d = [np.full((10, stride), 7, np.uint8) for _ in range(4)]
            if which == 0:
                RL.oc_frag_recon_intra_c(p(d[0], off), stride, p(r))
                RL.oc_frag_recon_inter_c(p(d[1], off), p(s1, off), stride, p(r))
                RL.oc_frag_recon_inter2_c(p(d[2], off), p(s1, off), p(s2, off), stride, p(r))
                RL.oc_frag_copy_c(p(d[3], off), p(s1, off), stride)
            else:
                OL.orc_frag_recon_intra(p(d[0], off), stride, p(r))
                OL.orc_frag_recon_inter(p(d[1], off), p(s1, off), stride, p(r))
                OL.orc_frag_recon_inter2(p(d[2], off), p(s1, off), p(s2, off), stride, p(r))
                OL.orc_frag_copy(p(d[3], off), p(s1, off), stride)
            outs.append(d)
        for a, b in zip(*outs):
            assert np.array_equal(a, b), k
    refcmp.TALLY["blocks"] += 4 * len(res)


def test_loop_filter_table_equals_the_reference_for_every_limit():
    refcmp.need_ref()
    for flimit in range(128):
        assert np.array_equal(ref.loop_filter_bv(flimit), oracle.loop_filter_bv(flimit)), flimit


@pytest.mark.parametrize("op", ["sad", "sad_thresh", "sad2_thresh", "intra_sad", "satd", "satd2", "intra_satd", "ssd"])
def test_metrics_equal_the_reference(op):
    refcmp.need_ref()
    g = _golden()
    if "enc_" + op in g.files:
        v, dc = ref.metric(op, g["enc_src"], g["enc_ref"], int(g["enc_stride"]), g["enc_so"], g["enc_ro"], g["enc_r2"], int(g["enc_thresh"]))
        assert np.array_equal(v, g["enc_" + op])
        if "enc_" + op + "_dc" in g.files:
            assert np.array_equal(dc, g["enc_" + op + "_dc"])
    for seed in (0, 1):
        src, rf = refcmp.pixel_planes(seed)
        h, w = src.shape
        so, ro, r2 = refcmp.block_offsets(seed, w, h, 400)
        plain, _ = ref.metric("sad2_thresh" if op == "sad2_thresh" else "sad", src, rf, w, so, ro, r2, 0xFFFFFFFF)
        threshes = [0]
        if "thresh" in op:     # below, at and above the results that occur
            threshes = [0, 1, int(np.median(plain)) - 1, int(np.median(plain)), int(np.median(plain)) + 1, int(plain.max()), int(plain.max()) + 1,
                        0xFFFFFFFF]
        for th in threshes:
            want = ref.metric(op, src, rf, w, so, ro, r2, th)
            got = oracle.enc_metric_batch(op, src, rf, w, so, ro, r2, th)
            assert np.array_equal(want[0], got[0]), (seed, th)
            if "satd" in op:
                assert np.array_equal(want[1], got[1]), (seed, th)
            refcmp.TALLY["blocks"] += len(so)


def test_sub_copy2_and_border_ssd_equal_the_reference():
    RL = refcmp.need_ref()
    OL = oracle.lib()
    src, rf = refcmp.pixel_planes(2)
    h, w = src.shape
    so, ro, r2 = refcmp.block_offsets(2, w, h, 300)
    rng = np.random.default_rng(5)
    masks = [0, -1, 1, 1 << 63, 1 << 36] + [int(rng.integers(-2 ** 63, 2 ** 63)) for _ in range(20)] + [(1 << k) - 1 for k in (8, 32, 56)]
    masks = [m - (1 << 64) if m >= 1 << 63 else m for m in masks]
    a = lambda arr, off=0: C.c_void_p(arr.ctypes.data + int(off))   # noqa: E731
    for i in range(len(so)):
        d = [np.zeros(64, np.int16) for _ in range(4)]
        RL.oc_enc_frag_sub_c(a(d[0]), a(src, so[i]), a(rf, ro[i]), w)
        OL.orc_enc_frag_sub(a(d[1]), a(src, so[i]), a(rf, ro[i]), w)
        RL.oc_enc_frag_sub_128_c(a(d[2]), a(src, so[i]), w)
        OL.orc_enc_frag_sub_128(a(d[3]), a(src, so[i]), w)
        assert np.array_equal(d[0], d[1]) and np.array_equal(d[2], d[3]), i
        c = [np.zeros((8, w), np.uint8) for _ in range(2)]
        RL.oc_enc_frag_copy2_c(a(c[0]), a(rf, ro[i]), a(rf, r2[i]), w)
        OL.orc_enc_frag_copy2(a(c[1]), a(rf, ro[i]), a(rf, r2[i]), w)
        assert np.array_equal(c[0], c[1]), i
        m = masks[i % len(masks)]
        assert RL.oc_enc_frag_border_ssd_c(a(src, so[i]), a(rf, ro[i]), w, m) == OL.orc_enc_frag_border_ssd(a(src, so[i]), a(rf, ro[i]), w, m), (i, m)
    refcmp.TALLY["blocks"] += 4 * len(so)


def _default_setup():
    """The setup header the reference encoder writes by default, parsed."""
    e = ref.RefEncoder(64, 48, 0, quality=32)
    hdr = e.header_packets()
    e.close()
    return hdr, enc_ref.SetupParams(hdr[2])


def test_quantiser_equals_the_reference_for_every_table():
    """oc_enquant_table_init_c + oc_enc_quantize_c against the oracle's quantiser: the dequantisation tables of all 64 qi x 2 frame
    types x 3 planes of the default setup header, coefficients on, one below and one above each rounding threshold."""
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    e = Encoder(64, 48, 0, 32)
    ours = enc_ref.SetupParams(e.header_packets()[2])       # and the tables th_encode_* itself writes and quantises with
    e.close()
    rng = np.random.default_rng(9)
    seen = set()
    for setup in (_default_setup()[1], ours):
        for qi in range(64):
            for qti in range(2):
                for pli in range(3):
                    dq = setup.qmat(qti, pli, qi)[refcmp.ZIGZAG].astype(np.uint16)
                    key = dq.tobytes()
                    if key in seen:
                        continue                    # (the same table again: the chroma planes share theirs)
                    seen.add(key)
                    x = refcmp.quant_inputs(dq, rng, nrandom=2)
                    want, wnz = ref.quantize(x, dq)
                    got, gnz = oracle.quantize_batch(x, dq)
                    bad = np.nonzero((want != got).any(axis=1) | (wnz != gnz))[0]
                    assert bad.size == 0, (qi, qti, pli, bad[:4])
                    refcmp.TALLY["blocks"] += len(x)
    assert len(seen) >= 128              # (many of the 384 coincide: chroma planes share tables, steps bottom out at high qi)


def test_our_info_header_is_the_references():
    """For the same th_info, th_encode_flushheader's info packet is the reference encoder's byte for byte.  (The setup packet is our
    own: other matrices and trees, which the format allows; test_quantiser_equals_the_reference_for_every_table covers its tables.)"""
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    hdr, _ = _default_setup()
    e = Encoder(64, 48, 0, 32)
    ours = e.header_packets()
    e.close()
    assert ours[0] == hdr[0]


# ---- whole streams: the generator's -------------------------------------------------------------------------------------------------
def _generated(w, h, fmt, seed, nframes, knobs=None):
    st = streamgen.Stream(w, h, fmt, seed=seed)
    st.setup.lflims[0:4] = [127] * 4            # the largest limit a setup header can carry, and none at all
    st.setup.lflims[60:64] = [0] * 4
    for k, v in (knobs or {}).items():
        setattr(st, k, v)
    hdr = st.header_packets()
    packets, truths = [], []
    for f in range(nframes):
        if f == 3:
            packets.append(b"")                 # a dropped frame
            truths.append(None)
            continue
        kw = dict(density=[0.9, 0.5, 0.15][f % 3])
        if f == 1:
            kw["force_qis"] = [2]               # loop-filter limit 127
        elif f == 2:
            kw["force_qis"] = [61, 5, 40]       # limit 0, three qi
        elif f == 6:
            kw["density"] = 0.0                 # nothing coded: a duplicate that is not an empty packet
        else:
            kw["nqis"] = 1 + f % 3
        pkt, truth = st.frame(0 if f % 5 == 0 else 1, **kw)
        packets.append(pkt)
        truths.append(None if truth["dup"] else (lambda o, t=truth: st.oracle_inputs(t, o)))
    return hdr, packets, truths


# 208x112 in 4:2:0 has chroma planes of 13 x 7 fragments: super-block rows and columns with a remainder of 1 and of 3 fragments
@pytest.mark.parametrize("fmt", [0, 2, 3])
@pytest.mark.parametrize("w,h,n", [(16, 16, 10), (64, 48, 10), (176, 144, 8), (208, 112, 8)])
def test_generated_streams_decode_like_the_reference(w, h, fmt, n):
    """Key and inter frames, all eight modes, both vector codings, 1..3 qi a frame, custom matrices and Huffman trees, loop-filter
    limits 0 and 127, dropped frames: reference decoder == oracle (ground truth) == oracle (front end's slot calls), and the two
    th_decode_packetin agree on return code and granule position."""
    refcmp.need_ref()
    hdr, packets, truths = _generated(w, h, fmt, seed=w * 3 + h + fmt, nframes=n)
    bad, pics = refcmp.compare_stream(hdr, packets, w, h, fmt, truths)
    assert not bad, bad[:4]
    assert len(pics) == n


@pytest.mark.parametrize("w,h,fmt", [(16, 16, 0), (64, 48, 2), (32, 48, 3)])
def test_vectors_far_outside_the_frame(w, h, fmt):
    """Every vector component +-31 or +-30 half pels: on these frames most predictors lie wholly or partly outside."""
    refcmp.need_ref()
    hdr, packets, truths = _generated(w, h, fmt, seed=77 + fmt, nframes=8, knobs=dict(mv_choices=[-31, 31, -30, 30, 17],
                                                                                     mode_choices=[2, 3, 4, 6, 7, 0]))
    bad, _ = refcmp.compare_stream(hdr, packets, w, h, fmt, truths)
    assert not bad, bad[:4]


# ---- whole streams: the reference encoder's ---------------------------------------------------------------------------------------
REF_ENCODED = [   # (name, w, h, fmt, pic, content, frames, encoder arguments)
    ("config1", 176, 144, 0, None, "lcg", 30, dict(quality=32, kf_interval=64)),
    ("dense", 176, 144, 0, None, "lcg_t", 6, dict(quality=32, kf_interval=64)),
    ("422", 80, 48, 2, None, "natural", 12, dict(quality=32, kf_interval=64)),
    ("444", 48, 64, 3, None, "natural", 12, dict(quality=32, kf_interval=64)),
    ("odd_region", 80, 64, 0, (3, 5, 61, 43), "natural", 10, dict(quality=32, kf_interval=64)),
    ("odd_region_444", 48, 48, 3, (1, 3, 45, 41), "natural", 6, dict(quality=40, kf_interval=64)),
    ("q0", 64, 48, 0, None, "natural", 8, dict(quality=0, kf_interval=64)),
    ("q16", 64, 48, 0, None, "noise", 8, dict(quality=16, kf_interval=64)),
    ("q48", 64, 48, 0, None, "natural", 8, dict(quality=48, kf_interval=64)),
    ("q63", 64, 48, 0, None, "natural", 8, dict(quality=63, kf_interval=64)),
    ("bitrate", 176, 144, 0, None, "natural", 24, dict(quality=0, bitrate=120000, kf_interval=64)),
    ("all_key", 64, 48, 0, None, "natural", 6, dict(quality=32, kf_interval=1)),
]


def _content(kind, w, h, fmt, n, seed=0):
    if kind.startswith("lcg"):
        return refcmp.lcg_frames(w, h, fmt, n, temporal=kind == "lcg_t")
    return refcmp.moving(kind, w, h, fmt, n, seed)


@pytest.mark.parametrize("name,w,h,fmt,pic,kind,n,kw", REF_ENCODED, ids=[c[0] for c in REF_ENCODED])
def test_reference_encoded_streams(name, w, h, fmt, pic, kind, n, kw):
    """Streams with an encoder's statistics: reference encoder -> front end (slot trace) -> oracle == reference decoder."""
    refcmp.need_ref()
    hdr, pk = refcmp.ref_encode(_content(kind, w, h, fmt, n, seed=len(name)), w, h, fmt, pic=pic, **kw)
    packets = [p for p, _ in pk]
    assert len(packets) == n
    bad, pics = refcmp.compare_stream(hdr, packets, w, h, fmt)
    assert not bad, bad[:4]
    keys = [not (p[0] & 0x40) for p in packets if p]
    assert keys[0] and (all(keys) if kw["kf_interval"] == 1 else not all(keys))     # (the reference may add key frames of its own)
    if name == "bitrate":
        assert any(refcmp.more_than_one_qi(p) for p in packets)       # several qi a frame occur
    if name == "config1":
        assert len(set(refcmp.digest(p) for p in pics)) == n    # (the pictures move: nothing is compared with a still)


# ---- our headers through the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,fmt,pic,fps,shift", [
    (64, 48, 0, (1, 2, 61, 45), (30000, 1001), 6), (176, 144, 2, None, (25, 1), 0), (32, 32, 3, (0, 5, 31, 27), (24, 1), 31),
])
def test_our_headers_parse_in_the_reference(w, h, fmt, pic, fps, shift):
    """The cases of test_encoder_cpu.py::test_headers_round_trip_through_decoder: th_encode_flushheader's packets parse with the
    reference's th_decode_headerin, and every th_info field equals what our own th_decode_headerin reads."""
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    RL = refcmp.need_ref()
    e = Encoder(w, h, fmt, 20, pic=pic, fps=fps, kfgshift=shift, comments=["TITLE=enc", "ARTIST=hip encoder"])
    hdr = e.header_packets()
    rcs, info, setup, tc = ref.headerin(hdr)
    try:
        assert rcs == [3, 2, 1]
        with refcmp.trace_mode():
            d = Decoder(hdr)
            ours = {k: int(getattr(d.info, k)) for k, _ in d.info._fields_}
            d.close()
        assert info.as_dict() == ours
        x, y, pw, ph = pic if pic else (0, 0, w, h)
        assert (info.frame_width, info.frame_height, info.pic_x, info.pic_y, info.pic_width, info.pic_height) == (w, h, x, y, pw, ph)
        assert (info.fps_numerator, info.fps_denominator, info.keyframe_granule_shift, info.pixel_fmt, info.quality) == (*fps, shift, fmt, 20)
        assert [C.string_at(tc.user_comments[k], tc.comment_lengths[k]) for k in range(tc.comments)] == [b"TITLE=enc", b"ARTIST=hip encoder"]
        assert C.string_at(tc.vendor) == e._L.th_version_string()
        dec = RL.th_decode_alloc(C.byref(info), setup)          # and the setup header is one the reference can decode with
        assert dec
        RL.th_decode_free(dec)
    finally:
        RL.th_setup_free(setup)
        RL.th_comment_clear(C.byref(tc))
        e.close()


# ---- the encoder restatements through the reference ---------------------------------------------------------------------------------
def _through_reference(headers, packets, recons):
    """Every packet is taken by the reference decoder, and its picture is the reconstruction the restatement reports."""
    rd = ref.RefDecoder(headers)
    for f, (pkt, want) in enumerate(zip(packets, recons)):
        rc, gp = rd.packetin(pkt)
        assert rc == (0 if pkt else ref.TH_DUPFRAME), (f, rc)
        bad = refcmp.diff_planes(rd.ycbcr_out(), want)
        assert not bad, (f, bad)
        refcmp.TALLY["frames"] += 1
    rd.close()


@pytest.mark.parametrize("w,h,fmt,pic,quality,kind", [
    (64, 48, 0, None, 32, "natural"), (64, 48, 2, (1, 2, 61, 45), 40, "natural"), (32, 32, 3, (0, 5, 31, 27), 8, "noise"),
    (176, 144, 0, None, 20, "natural"), (16, 16, 0, None, 63, "noise"), (48, 32, 3, None, 0, "gradient")])
def test_intra_restatement_through_the_reference(w, h, fmt, pic, quality, kind):
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    e = Encoder(w, h, fmt, quality, pic=pic)
    hdr = e.header_packets()
    e.close()
    setup = enc_ref.SetupParams(hdr[2])
    p = pic or (0, 0, w, h)
    packets, recons = [], []
    ost = oracle.State(w, h, fmt)
    for seed in range(3):
        r = enc_ref.encode_frame(enc_ref.picture(kind, w, h, fmt, p, picture_size=pic is not None, seed=seed), w, h, fmt, p, quality, setup)
        assert enc_ref.oracle_decode(ost, r) == 0
        packets.append(r["packet"])
        recons.append([a.copy() for a in refcmp.oracle_picture(ost)])
    ost.close()
    _through_reference(hdr, packets, recons)


@pytest.mark.parametrize("which", ["five", "eight"])
@pytest.mark.parametrize("kind,w,h,fmt,q,kf", [("uncover", 176, 144, 0, 32, 64), ("shear", 176, 144, 0, 32, 4), ("pan", 64, 48, 2, 16, 3),
                                               ("shear", 48, 64, 3, 48, 64)])
def test_inter_restatements_through_the_reference(which, kind, w, h, fmt, q, kf):
    """enc_inter_ref.InterEncoder (five modes) and enc_modes_ref.ModesEncoder (eight modes, golden frames, four vectors): the rule
    include/theoraenc_hip.h states yields packets the reference decodes to exactly the reconstruction the restatement reports."""
    from tests import enc_inter_ref as IR
    from tests import enc_modes_ref as M
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    e = Encoder(w, h, fmt, q)
    hdr = e.header_packets()
    e.close()
    enc = (IR.InterEncoder if which == "five" else M.ModesEncoder)(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), kf, 6)
    packets, recons, m8 = [], [], np.zeros(8, np.int64)
    for fr in M.sequence(kind, w, h, fmt, 8):
        r = enc.frame(fr, q)
        packets.append(r["packet"])
        recons.append(enc.recon)
        if "modes8" in r and not r["key"]:
            m8 += r["modes8"]
    enc.close()
    _through_reference(hdr, packets, recons)
    if which == "eight" and kind == "uncover":
        assert m8[5] + m8[6] > 0          # golden modes were in what the reference decoded
    if which == "eight" and kind == "shear" and w == 176:
        assert m8[7] > 0                  # and four-vector macro blocks


@pytest.mark.parametrize("q,delta", [(32, 8), (0, 6), (63, 10), (60, 12), (2, 31)])
@pytest.mark.parametrize("kind", ["key", "five", "eight"])
def test_block_qi_restatement_through_the_reference(kind, q, delta):
    """The cases of test_encoder_bqi_cpu.py::test_restatement_packets_decode_to_its_reconstruction, through the reference."""
    from tests import enc_bqi_ref as B
    from tests import enc_modes_ref as M
    from theora_amd.encoder import Encoder
    refcmp.need_ref()
    w, h, fmt = 64, 48, 0
    e = Encoder(w, h, fmt, q)
    hdr = e.header_packets()
    e.close()
    enc = B.BqiEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 1 if kind == "key" else 64, 6, delta, modes=kind == "eight")
    packets, recons = [], []
    for fr in M.sequence("shear" if kind == "eight" else "pan", w, h, fmt, 4, seed=q + delta):
        packets.append(enc.frame(fr, q)["packet"])
        recons.append(enc.recon)
    enc.close()
    assert any(refcmp.more_than_one_qi(p) for p in packets)
    _through_reference(hdr, packets, recons)


# ---- post-processing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("w,h,fmt", [(64, 48, 0), (176, 144, 0), (48, 64, 3), (80, 48, 2)])
def test_postprocessing_equals_the_reference(w, h, fmt, level):
    """TH_DECCTL_SET_PPLEVEL in the reference decoder against oracle.State.postprocess on a coarsely quantised stream (the filters
    act where the quantiser is coarse), the DC quantiser indices tracked per fragment as the decoder does."""
    refcmp.need_ref()
    st = streamgen.Stream(w, h, fmt, seed=w + h + fmt)
    st.max_mag = 40
    hdr = st.header_packets()
    rd = ref.RefDecoder(hdr)
    assert rd.pp_level_max() == 7
    rd.set_pp_level(level)
    dcs, shm = refcmp.pp_tables(st.setup)
    ost = oracle.State(w, h, fmt)
    n = ost.nfrags
    dc_qis, qii_persist, qis_persist = None, np.zeros(n, np.int64), [0, 0, 0]
    changed = 0
    for f in range(6):
        pkt, truth = st.frame(0 if f % 4 == 0 else 1, density=[0.9, 0.5, 0.3][f % 3], force_qis=[[3], [9, 1], [0, 14, 5]][f % 3])
        rc, _ = rd.packetin(pkt)
        assert rc == (1 if truth["dup"] else 0)
        if not truth["dup"]:
            assert ost.decode_frame(**st.oracle_inputs(truth, ost)) == 0
            cf = truth["coded_fragis"]
            for k, q in enumerate(truth["qis"]):
                qis_persist[k] = int(q)
            qii_persist[cf] = truth["qii"][cf]
            if dc_qis is None:
                dc_qis = np.full(n, truth["qis"][0], np.uint8)
            else:
                dc_qis[cf] = truth["qis"][0]
            plain = [ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
            if level >= 2:
                frag_qi = np.array(qis_persist, np.uint8)[qii_persist]
                want, _ = ost.postprocess(oracle.FRAME_PREV, level, truth["flimit"] != 0, dc_qis, frag_qi, dcs, shm)
            else:
                want = plain
            changed += sum(int((a != b).sum()) for a, b in zip(want, plain))
        bad = refcmp.diff_planes(rd.ycbcr_out(), [a[::-1] for a in want])
        assert not bad, (f, bad)
        refcmp.TALLY["frames"] += 1
    assert (changed > 0) == (level >= 2)          # the filters did act
    rd.close()
    ost.close()


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
def test_the_comparison_notices_one_altered_value():
    """The comparison itself: the same stream with the oracle's input altered in one place -- the loop-filter limit of one frame
    plus one; one vector of one frame off by half a pel -- must be reported, and is not without the alteration."""
    refcmp.need_ref()
    w, h, fmt = 64, 48, 0
    hdr, pk = refcmp.ref_encode(refcmp.moving("noise", w, h, fmt, 5, seed=4), w, h, fmt, quality=24, kf_interval=64)
    packets = [p for p, _ in pk]
    assert not refcmp.compare_stream(hdr, packets, w, h, fmt)[0]

    def limit_plus_one(f, t):
        if f == 1:
            assert t["flimit"] > 0
            t["flimit"] += 1

    def half_a_pel(f, t):
        if f == 2:
            k = np.nonzero(t["refi"] != oracle.FRAME_SELF)[0]
            assert k.size
            t["mv"][k[0]] ^= 1          # the x component's lowest bit

    for alter in (limit_plus_one, half_a_pel):
        bad, _ = refcmp.compare_stream(hdr, packets, w, h, fmt, alter=alter)
        assert bad and all(b[1] == "front end -> oracle != reference" for b in bad), (alter.__name__, bad[:3])
        assert bad[0][0] == (1 if alter is limit_plus_one else 2)


# ---- the fixture: something the reference made, on every machine --------------------------------------------------------------------
def test_fixture_decodes_to_the_references_digests():
    """tests/golden/ref_qcif_q32.npz: QCIF, 30 frames, quality 32, made by the reference encoder, with the reference decoder's digest
    of every frame.  Needs neither oracle/_ref/ nor the reference tree: front end (slot trace) -> oracle."""
    from theora_amd.decoder import Decoder
    hdr, packets, gps, digests = refcmp.load_fixture()
    assert len(packets) == 30 == len(digests)
    with refcmp.trace_mode():
        dec = Decoder(hdr)
        ost = oracle.State(176, 144, 0)
        for f, pkt in enumerate(packets):
            rc, gp = dec.packetin(pkt)
            assert (rc, gp) == (0, gps[f]), f
            assert refcmp.oracle_apply_trace(ost, dec.slot_trace()) == 0
            assert refcmp.digest(refcmp.oracle_picture(ost)) == digests[f], f
        dec.close()
        ost.close()


def test_fixture_is_what_the_reference_makes_today():
    """Where the library is: the reference encoder on the same content gives the fixture's packets, the reference decoder its digests."""
    refcmp.need_ref()
    hdr, packets, gps, digests = refcmp.load_fixture()
    rh, pk = refcmp.ref_encode(refcmp.lcg_frames(176, 144, 0, 30), 176, 144, 0, quality=32, kf_interval=64)
    assert rh == hdr and [p for p, _ in pk] == packets and [g for _, g in pk] == gps
    rd = ref.RefDecoder(hdr)
    for f, pkt in enumerate(packets):
        assert rd.packetin(pkt) == (0, gps[f])
        assert refcmp.digest(rd.ycbcr_out()) == digests[f], f
    rd.close()
