"""A caller's quantisation parameters in th_encode_* (include/theoraenc_hip.h, "Quantisation parameters") without a GPU:
th_encode_alloc, th_encode_ctl and th_encode_flushheader never touch it, and thip_quant_info_from_setup is host code.

Request 2 and 0x7229 (refusals, timing, validity), the setup header of every family of tests/enc_quant_ref.py (against the
restatement's packer, this library's and the reference's th_decode_headerin, the reference encoder's own header),
thip_quant_info_from_setup (round trips, the reference's own quantiser bits, truncated and corrupt packets),
tests/native/quant_host.cpp under the sanitizers, the rate probe's floor, and the restatements' streams under foreign parameters in
this library's front end and the reference decoder."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_inter_ref, enc_modes_ref, enc_ref, quant_host, refcmp
from tests import enc_quant_ref as QR

W, H = 64, 48
TH_EBADHEADER, TH_ENOTFORMAT = -20, -21   # include/theoradec_hip.h


def _E():
    from theora_amd import encoder as E
    return E


def _enc(**kw):
    return _E().Encoder(W, H, 0, 32, **kw)


@pytest.fixture(scope="module")
def fams():
    return QR.families()


@pytest.fixture(scope="module")
def plain():
    e = _enc()
    hdr, q = e.header_packets(), e.quant_params()
    e.close()
    return hdr, q


def _set(e, p, size=None):
    """th_encode_ctl(request 2) with the Params as they are -> the return code."""
    s = p.quant_info().struct()
    return e._L.th_encode_ctl(e._enc, 2, C.byref(s), C.sizeof(s) if size is None else size)


def _invalid(fams):
    """One set a kind, each wrong in one place only -> {kind: (Params, the (qti, pli) with NULL arrays)}."""
    out = {}
    p = fams["ranges"].copy()
    p.sizes[1][2] = [1, 31, 30]
    out["sizes sum to 62"] = (p, ())
    p = fams["ranges"].copy()
    p.sizes[0][1] = [1, 31, 32]
    out["sizes sum to 64"] = (p, ())
    p = fams["ranges"].copy()
    p.sizes[0][0] = [0, 32, 31]
    out["a size of 0"] = (p, ())
    p = fams["ranges"].copy()
    p.sizes[1][0] = [-1, 33, 31]
    out["a negative size"] = (p, ())
    p = fams["shared"].copy()
    p.sizes[0][2], p.mats[0][2] = [], p.mats[0][2][:1]
    out["no range"] = (p, ())
    p = fams["edge-low"].copy()
    p.sizes[0][0], p.mats[0][0] = [1] * 64, np.concatenate([p.mats[0][0], p.mats[0][0][:1]])
    out["64 ranges"] = (p, ())
    p = fams["saw"].copy()
    p.lf[17] = 128
    out["a limit of 128"] = (p, ())
    out["NULL arrays"] = (fams["saw"].copy(), ((1, 1),))
    return out


def _struct_with_nulls(p, null):
    s = p.quant_info().struct()
    for qti, pli in null:
        s.qi_ranges[qti][pli].sizes = None
        s.qi_ranges[qti][pli].base_matrices = None
    return s


def test_set_with_a_full_size_buffer(fams):
    """The test that shows the feature: request 2 with a th_quant_info answers 0 (it was TH_EIMPL), 0x7229 returns what was set,
    and the header carries it."""
    E = _E()
    assert C.sizeof(E.QuantInfoStruct) == 464
    e = _enc()
    try:
        assert _set(e, fams["ranges"]) == 0
        assert fams["ranges"].same(e.quant_params())
        got = QR.from_setup(enc_ref.SetupParams(e.header_packets()[2]))
        assert fams["ranges"].same(got.quant_info())
    finally:
        e.close()


def test_request_2_refusals_and_timing(fams, plain):
    from theora_amd import _lib as Lm
    E = _E()
    saw, ranges = fams["saw"], fams["ranges"]
    e = _enc()
    try:
        v = C.c_int(0)
        assert e._L.th_encode_ctl(e._enc, 2, C.byref(v), 4) == Lm.EIMPL      # the probe with an int
        for size in (0, 4, 463, 465, 472):
            assert _set(e, saw, size) == Lm.EIMPL, size
        assert e._L.th_encode_ctl(e._enc, 2, None, 464) == Lm.EIMPL
        assert e.quant_params() == plain[1]
        assert _set(e, saw) == 0 and saw.same(e.quant_params())
        for kind, (bad, null) in _invalid(fams).items():
            assert null or not QR.valid(bad), kind
            s = _struct_with_nulls(bad, null)
            assert e._L.th_encode_ctl(e._enc, 2, C.byref(s), C.sizeof(s)) == Lm.EINVAL, kind
            assert saw.same(e.quant_params()), kind                           # the parameters stay as they were
        assert e._L.th_encode_ctl(e._enc, 2, None, 0) == 0                    # the built-in parameters again
        assert e.quant_params() == plain[1] and e.header_packets() == plain[0]
        # too late: a header packet has gone out
        assert _set(e, saw) == Lm.EINVAL and e._L.th_encode_ctl(e._enc, 2, None, 0) == Lm.EINVAL
        assert e.quant_params() == plain[1]
        s = E.QuantInfoStruct()
        assert e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_GET_QUANT_PARAMS, C.byref(s), 463) == Lm.EINVAL
        assert e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_GET_QUANT_PARAMS, None, 464) == Lm.EINVAL
    finally:
        e.close()
    e = _enc()
    try:   # after the FIRST header packet, not the last
        op, tc = Lm.OggPacket(), Lm.ThComment()
        e._L.th_comment_init(C.byref(tc))
        assert _set(e, ranges) == 0
        assert e._L.th_encode_flushheader(e._enc, C.byref(tc), C.byref(op)) == 1
        assert _set(e, saw) == Lm.EINVAL
        assert ranges.same(e.quant_params())
    finally:
        e.close()
    with pytest.raises(ValueError):
        _enc(quant=_invalid(fams)["sizes sum to 62"][0].quant_info())


def test_the_copy_is_deep_and_get_may_be_set_back(fams):
    """The caller's arrays go away after SET; what GET hands out points into the context and may be given to SET itself."""
    E = _E()
    e = _enc()
    try:
        qi = fams["ranges"].quant_info()
        s = qi.struct()
        assert e._L.th_encode_ctl(e._enc, 2, C.byref(s), C.sizeof(s)) == 0
        for keep in qi._keep[1]:
            C.memset(keep, 0xA5, C.sizeof(keep))
        qi._keep = None
        assert fams["ranges"].same(e.quant_params())
        g = E.QuantInfoStruct()
        assert e._L.th_encode_ctl(e._enc, E.TH_ENCCTL_THIP_GET_QUANT_PARAMS, C.byref(g), C.sizeof(g)) == 0
        assert e._L.th_encode_ctl(e._enc, 2, C.byref(g), C.sizeof(g)) == 0     # the context's own arrays as the source
        assert fams["ranges"].same(e.quant_params())
    finally:
        e.close()


def test_python_layer(fams, plain):
    E = _E()
    e = E.Encoder(W, H, 0, 32, quant=fams["saw"].quant_info())
    assert fams["saw"].same(e.quant_params())
    e.set_quant_params(None)
    assert e.quant_params() == plain[1]
    e.set_quant_params(fams["shared"].quant_info())
    hdr = e.header_packets()
    e.close()
    assert fams["shared"].same(E.quant_from_headers(hdr))
    with pytest.raises(ValueError):
        E.quant_from_headers(hdr[:2])


def _huff_tail(plain_hdr):
    return QR.quant_bits_of_packet(plain_hdr[2])[1]


def test_setup_packets_of_every_family(fams, plain, tmp_path_factory, tmp_path):
    from oracle import ref
    from theora_amd.decoder import Decoder
    E = _E()
    tail = _huff_tail(plain[0])
    steps = quant_host.Steps()
    seen = set()
    for name, p in fams.items():
        assert QR.valid(p), name
        steps.set(p)
        e = _enc(quant=p.quant_info())
        hdr = e.header_packets()
        e.close()
        want_bits, codes = QR.pack_bits(p)
        seen.update(codes)
        assert hdr[2] == QR.setup_packet(p, tail), name           # the restatement's packet, the Huffman part unchanged
        assert hdr[:2] == plain[0][:2], name
        assert p.same(QR.from_setup(enc_ref.SetupParams(hdr[2])).quant_info()), name
        # this library's th_decode_headerin takes it (the front end's tables are checked through a frame below)
        with refcmp.trace_mode():
            Decoder(hdr).close()
        if ref.available():
            rcs, info, setup, tc = ref.headerin(hdr)
            RL = ref.lib()
            RL.th_setup_free(setup)
            RL.th_comment_clear(C.byref(tc))
            assert all(rc > 0 for rc in rcs), (name, rcs)
            # the reference encoder, given the same th_quant_info and our codes, writes the same setup packet byte for byte
            r = ref.RefEncoder(W, H, 0, quality=32)
            s = p.quant_info().struct()
            assert r._L.th_encode_ctl(r._enc, 2, C.byref(s), C.sizeof(s)) == 0, name
            pe = _enc()
            buf = E._huff_codes_in(pe.huffman_codes())
            pe.close()
            assert r._L.th_encode_ctl(r._enc, 0, C.byref(buf), C.sizeof(buf)) == 0
            rh = r.header_packets()
            r.close()
            assert rh[2] == hdr[2], name
    assert seen == {"0", "00", "01", "1"}
    assert QR.pack_bits(fams["shared"])[1] == ["0", "0", "01", "01", "01"]
    assert QR.pack_bits(fams["shared-variant"])[1] == ["1", "0", "00", "01", "01"]
    # a copy of the built-in values: the same parameters, a header that differs in the duplicate codes only
    e = _enc(quant=plain[1])
    hdr = e.header_packets()
    e.close()
    assert hdr[2] != plain[0][2] and e is not None
    a, b = enc_ref.SetupParams(hdr[2]), enc_ref.SetupParams(plain[0][2])
    assert all(np.array_equal(a.qmat(t, pl, q), b.qmat(t, pl, q)) for t, pl in QR.PAIRS for q in (0, 17, 63))
    assert a.lflims == b.lflims and a.codes == b.codes
    # the stand-alone program under the sanitizers: clean, its bits the library's, its floor steps.min(axis=q)
    inv = _invalid(fams)
    for kind, (bad, null) in inv.items():
        steps.set(bad, null)
    got = steps.run(quant_host.build(tmp_path_factory), tmp_path)
    for (name, p), g in zip(fams.items(), got):
        assert g["valid"] == 1 and g["again"] == 1 and g["steps_ok"] == 1, name
        assert g["bits"] == QR.pack_bits(p)[0], name
        assert g["nbms"] == len(QR.consolidate(p)[0]), name
        assert np.array_equal(g["floor"], QR.floor(QR.steps(p))), name
    for kind, g in zip(inv, got[len(fams):]):
        assert g["valid"] == 0, kind


def test_floor_and_range(fams):
    """rate_form_floor is steps.min(axis=q); under `saw` the least step is mostly not at qi 63, and for the DC only at q = 0.  Every
    step of every family is in 1..32767 (the range part of rate_steps_ok, which the stand-alone program prints as steps_ok)."""
    st = QR.steps(fams["saw"]).astype(np.int64)
    fl = QR.floor(st)
    assert (st[:, 63, :] > fl).mean() > 0.5
    only0 = (st[:, 0, :] == fl) & ((st[:, 1:, :] > fl[:, None, :]).all(axis=1))
    assert only0[:, 0].all() and not only0[:, 1:].any()
    e = _enc()
    b = QR.steps(QR.from_setup(enc_ref.SetupParams(e.header_packets()[2])))
    e.close()
    assert np.array_equal(QR.floor(b), b[:, 63, :])               # the built-in tables: the floor IS column 63
    for name, p in fams.items():
        s = QR.steps(p)
        assert s.min() >= 8 and s.max() <= 4096, name
    # the library's range check and the old call form, through thip_enc_rate_stage: every refusal comes before a device is touched
    # (the addresses are never read).  The library's rate_form_floor itself is held against steps.min(axis=q) through
    # tests/native/quant_host.cpp in test_setup_packets_of_every_family.
    from theora_amd import _lib as Lm
    from theora_amd.encoder import rate_stage

    def stage(steps, **kw):
        return rate_stage((16, 16), 0, 0, 2, steps=steps, coef=4096, qdc=8192, **kw)
    saw = QR.steps(fams["saw"])
    assert stage(saw) == Lm.EINVAL and stage(saw, any_order=0) == Lm.EINVAL      # a step below that of qi 63
    assert stage(saw, any_order=2) == Lm.EINVAL and stage(saw, any_order=-1) == Lm.EINVAL
    for t, q, z, v in ((0, 0, 0, 0), (5, 63, 63, 0), (3, 7, 9, 32768), (2, 63, 1, 65535)):
        bad = saw.copy()
        bad[t, q, z] = v
        assert stage(bad, any_order=1) == Lm.EINVAL, (t, q, z, v)
        assert stage(bad, any_order=0) == Lm.EINVAL, (t, q, z, v)
    # (steps in range with any_order = 1 pass this check and reach the device: tests/test_gpu_rate_quant_direct.py)


def test_quant_info_from_setup(fams, plain):
    from theora_amd import _lib as Lm
    from theora_amd.decoder import Decoder
    E = _E()
    L = Lm.load()
    # the reference-made packet: parse -> SET -> header reproduces its quantiser bits exactly
    pkt = QR.ref_setup_packet()
    q = E.quant_from_setup(pkt)
    assert fams["ref"].same(q)
    e = _enc(quant=q)
    hdr = e.header_packets()
    e.close()
    assert QR.quant_bits_of_packet(hdr[2])[0] == QR.quant_bits_of_packet(pkt)[0]
    # a round trip of every family, and of the built-in header
    for name, p in fams.items():
        assert p.same(E.quant_from_setup(QR.setup_packet(p, _huff_tail(plain[0])))), name
    assert E.quant_from_setup(plain[0][2]) == plain[1]
    # NULLs
    s = E.QuantInfoStruct()
    assert L.thip_quant_info_from_setup(None, 10, C.byref(s)) == Lm.EFAULT and L.thip_quant_info_from_setup(pkt, len(pkt), None) == Lm.EFAULT
    L.thip_quant_info_free(None)
    L.thip_quant_info_free(C.byref(s))      # zeroed: fine
    # truncated and corrupt packets answer as th_decode_headerin does for the same bytes as a stream's third header
    cases = [pkt[:0], pkt[:1], pkt[:6], pkt[:7], pkt[:40], pkt[:len(pkt) // 2], pkt[:-40], b"\x82theorb" + pkt[7:], b"\x82vorbis" + pkt[7:],
             plain[0][0], plain[0][1], b"\x83theora" + pkt[7:], b"\x00" + pkt[1:], pkt[:7] + b"\xff" * 200, pkt]
    for k, bad in enumerate(cases):
        s = E.QuantInfoStruct()
        got = L.thip_quant_info_from_setup(bad if bad else b"\x00", len(bad), C.byref(s))
        L.thip_quant_info_free(C.byref(s))
        info, tc, setup = Lm.ThInfo(), Lm.ThComment(), C.c_void_p()
        L.th_info_init(C.byref(info))
        L.th_comment_init(C.byref(tc))
        rcs = []
        for n, h in enumerate([plain[0][0], plain[0][1], bad]):
            op = Lm.OggPacket()
            data = (C.c_ubyte * max(len(h), 1)).from_buffer_copy(h if h else b"\x00")
            op.packet, op.bytes, op.b_o_s, op.packetno = C.addressof(data), len(h), int(n == 0), n
            rcs.append(L.th_decode_headerin(C.byref(info), C.byref(tc), C.byref(setup), C.byref(op)))
        L.th_setup_free(setup)
        L.th_comment_clear(C.byref(tc))
        L.th_info_clear(C.byref(info))
        assert rcs[:2] == [3, 2], k
        assert got == (0 if rcs[2] > 0 else rcs[2]) and (got == 0) == (k == len(cases) - 1), (k, got, rcs)
        assert got in (0, TH_ENOTFORMAT, TH_EBADHEADER), (k, got)
    with refcmp.trace_mode():
        Decoder(hdr).close()


def _pictures(hdr, packets, recons):
    """The packets through the reference decoder where it is present: its pictures equal the restatement's reconstructions."""
    from oracle import ref
    if not ref.available():
        return
    rd = ref.RefDecoder(hdr)
    for n, (pkt, want) in enumerate(zip(packets, recons)):
        assert rd.packetin(pkt)[0] >= 0, n
        assert not refcmp.diff_planes(rd.ycbcr_out(), want), n
    rd.close()


@pytest.mark.parametrize("name", ["ref", "ranges", "saw", "shared", "shared-variant", "edge-low", "edge-high"])
def test_restatements_under_foreign_parameters(fams, name):
    """tests/enc_ref.py, enc_inter_ref.py and enc_modes_ref.py build every table from the stream's own setup header: their streams
    under every family.  th_decode_headerin's tables are spec 6.4.3 over the INPUT parameters: the front end (slot-trace mode, no
    device) dequantises a key frame at qi 0, 31 and 63 with the intra steps restated from the input and takes the input's
    loop-filter limit, and its slot calls for inter streams, fed to the oracle, give the restatement's reconstruction (the inter
    steps).  The reference decoder's pictures are the restatement's reconstructions too."""
    import oracle
    from theora_amd.decoder import Decoder
    p = fams[name]
    e = _enc(quant=p.quant_info())
    hdr = e.header_packets()
    e.close()
    setup = enc_ref.SetupParams(hdr[2])
    pic = (0, 0, W, H)
    for qi in (0, 31, 63):
        fr = enc_ref.picture("natural", W, H, 0, seed=qi)
        r = enc_ref.encode_frame(fr, W, H, 0, pic, qi, setup)
        for pl in range(3):
            assert np.array_equal(r["dequant"][pl], QR.qmat(p, 0, pl, qi)[enc_ref.ZIGZAG]), (qi, pl)
        with refcmp.trace_mode():
            dec = Decoder(hdr)
            assert dec.packetin(r["packet"])[0] == 0
            t = dec.slot_trace()
            dec.close()
        dq = r["dequant"][r["plane_of"]]
        want = np.zeros((len(r["coded_order"]), 64), np.int64)
        want[:, enc_ref.ZIGZAG] = r["levels"] * dq
        want[:, 0] = r["levels"][:, 0]
        assert np.array_equal(t["fragi"], r["coded_order"]) and np.array_equal(t["coeffs"], want), qi
        assert np.array_equal(t["dc_quant"], dq[:, 0]) and t["flimit"] == p.lf[qi], qi
        ost = oracle.State(W, H, 0)
        assert enc_ref.oracle_decode(ost, r) == 0
        _pictures(hdr, [r["packet"]], [refcmp.oracle_picture(ost)])
        ost.close()
    for cls, seq in ((enc_inter_ref.InterEncoder, enc_inter_ref.sequence), (enc_modes_ref.ModesEncoder, enc_modes_ref.sequence)):
        enc = cls(W, H, 0, pic, setup, 64, 6)
        packets, recons = [], []
        for planes in seq("pan", W, H, 0, 4, seed=3):
            r = enc.frame(planes, 30)
            packets.append(r["packet"])
            recons.append([a.copy() for a in enc.recon])
        enc.close()
        assert sum(len(pk) > 0 for pk in packets) >= 3
        with refcmp.trace_mode():
            dec, ost = Decoder(hdr), oracle.State(W, H, 0)
            for n, (pk, want) in enumerate(zip(packets, recons)):
                if dec.packetin(pk)[0] == 0:
                    assert refcmp.oracle_apply_trace(ost, dec.slot_trace()) == 0, n
                assert not refcmp.diff_planes(refcmp.oracle_picture(ost), want), (cls.__name__, n)
            dec.close()
            ost.close()
        _pictures(hdr, packets, recons)
