"""th_encode_*'s block-level qi without a GPU: the controls (TH_ENCCTL_THIP_SET_BLOCK_QI, TH_ENCCTL_THIP_GET_BLOCK_QI_STATS), and the
restatement of the rule (tests/enc_bqi_ref.py): its packets, parsed by the library's own front end (slot-trace mode, no device) and
fed to the oracle, give the restatement's own reconstruction.  Nothing here reaches the first th_encode_ycbcr_in."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import enc_bqi_ref as B
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


def test_block_qi_controls():
    """0 and 1..31 accepted, anything else TH_EINVAL; the call never touches the GPU (this machine may have none)."""
    from theora_amd import encoder as E
    assert (E.TH_ENCCTL_THIP_SET_BLOCK_QI, E.TH_ENCCTL_THIP_GET_BLOCK_QI_STATS) == (0x720B, 0x720C)
    assert C.sizeof(E.BlockQiStats) == 14 * 4
    L, enc = _enc()
    try:
        for d in (0, 1, 7, 31, 0):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, d) == (0, d)
        for d in (-1, 32, 64, 1 << 20, -(1 << 31)):
            assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, d)[0] == TH_EINVAL, d
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, None, 4) == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, 3, C.c_int64)[0] == TH_EINVAL
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_INTER_FRAMES, 1)[0] == 0
        assert _ctl(L, enc, E.TH_ENCCTL_THIP_SET_BLOCK_QI, 5) == (0, 5)
        s = E.BlockQiStats()
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_BLOCK_QI_STATS, C.byref(s), C.sizeof(s)) == 0
        assert s.nqis == 0 and s.flag_bits == 0 and list(s.qis) == [0, 0, 0]
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_THIP_GET_BLOCK_QI_STATS, C.byref(s), C.sizeof(s) - 4) == TH_EINVAL
        assert _ctl(L, enc, 0x7299, 0)[0] == TH_EIMPL   # (still pinned)
    finally:
        L.th_encode_free(enc)


def test_python_encoder_block_qi():
    from theora_amd.encoder import Encoder
    e = Encoder(64, 48, 0, 20, block_qi=4)
    assert e.block_qi == 4 and e.block_qi_stats()["nqis"] == 0
    e.close()
    with pytest.raises(ValueError):
        Encoder(64, 48, 0, 20, block_qi=32)


def test_headers_do_not_change_with_block_qi():
    from theora_amd.encoder import Encoder
    assert Encoder(64, 48, 0, 20).header_packets() == Encoder(64, 48, 0, 20, block_qi=9).header_packets()


def test_qi_list():
    assert B.qi_list(32, 0) == [32]
    assert B.qi_list(32, 8) == [32, 24, 40]
    assert B.qi_list(0, 8) == [0, 8]
    assert B.qi_list(3, 8) == [3, 0, 11]
    assert B.qi_list(63, 31) == [63, 32]
    assert B.qi_list(60, 8) == [60, 52, 63]


def test_ac_bits_counts_the_walk_from_index_one():
    bits = [[1] * 32 for _ in range(4)]   # one bit a token: R is the token count plus the extra bits
    lv = np.zeros(64, np.int64)
    assert B.ac_bits(lv, bits) == 1                      # an EOB at index 1
    lv[0] = 5
    assert B.ac_bits(lv, bits) == 1                      # the DC does not count
    lv[1] = 1
    assert B.ac_bits(lv, bits) == 2                      # +-1 (no extra bits), EOB
    lv[63] = -2
    assert B.ac_bits(lv, bits) == 1 + 1 + 6 + 1         # +-1; ZRL (6 extra bits) over 2..62; -2, no EOB


@pytest.fixture()
def trace_env():
    from theora_amd import _lib
    L = _lib.load()
    old = L.thip_option(b"fe_trace_backend")
    assert L.thip_set_option(b"fe_trace_backend", 1) == 0
    yield
    L.thip_set_option(b"fe_trace_backend", old)


def _decode_check(enc, headers, packets, recons, w, h, fmt):
    """Each packet through the front end (slot trace) and the oracle: the picture equals the restatement's reconstruction."""
    from theora_amd.decoder import Decoder
    dec = Decoder(headers)
    ost = oracle.State(w, h, fmt)
    try:
        for pkt, rec in zip(packets, recons):
            rc, _ = dec.packetin(pkt)
            if not pkt:
                assert rc == 1
                continue
            assert rc == 0
            got = dec.slot_trace()
            ost.refi[:] = oracle.FRAME_NONE
            ost.refi[got["fragi"]] = got["refi"]
            ost.mvs[:] = 0
            ost.mvs[got["fragi"]] = got["mv"]
            ncoded = [int((got["pli"] == p).sum()) for p in range(3)]
            assert ost.decode_frame(got["frame_type"], got["fragi"], ncoded, got["coeffs"], got["last_zzi"], got["dc_quant"],
                                    got["uncoded"], got["flimit"]) == 0
            for p in range(3):
                assert np.array_equal(ost.get_plane(oracle.FRAME_PREV, p)[::-1], rec[p]), p
    finally:
        dec.close()
        ost.close()


@pytest.mark.parametrize("q,delta,nqis", [(32, 0, 1), (32, 8, 3), (0, 6, 2), (63, 10, 2), (60, 12, 3), (2, 31, 3)])
@pytest.mark.parametrize("kind", ["key", "five", "eight"])
def test_restatement_packets_decode_to_its_reconstruction(trace_env, kind, q, delta, nqis):
    from theora_amd.encoder import Encoder
    w, h, fmt = 64, 48, 0
    headers = Encoder(w, h, fmt, q).header_packets()
    setup = enc_ref.SetupParams(headers[2])
    frames = M.sequence("shear" if kind == "eight" else "pan", w, h, fmt, 4, seed=q + delta)
    e = B.BqiEncoder(w, h, fmt, (0, 0, w, h), setup, 1 if kind == "key" else 64, 6, delta, modes=kind == "eight")
    packets, recons, used = [], [], set()
    for fr in frames:
        r = e.frame(fr, q)
        packets.append(r["packet"])
        recons.append(e.recon)
        if r["packet"]:
            assert r["bqi"]["nqis"] == nqis and r["bqi"]["qis"][:nqis] == B.qi_list(q, delta)
            used |= {k for k in range(3) if sum(r["bqi"]["blocks"][k])}
    e.close()
    if nqis == 3:
        assert len(used) >= 2, used   # the choice is not a constant on this content
    _decode_check(e, headers, packets, recons, w, h, fmt)
