"""th_encode_* with the level choice on the GPU (TH_ENCCTL_THIP_SET_RD_QUANT): the packets, the statistics and the reconstruction equal
tests/enc_rdq_ref.py's restatement byte for byte -- over enc_rdq_ref.PACKET_CASES (key-only and inter streams at 64 x 48 and
176 x 144, the three pixel formats, five and eight modes, block qi, masking, the rate-distortion mode decision, the skip decision;
tests/test_encoder_rdq_cpu.py asserts that none of them is vacuous) -- and so they do with the device packetiser, in bitrate mode, with
automatic key frames and with device input the caller overwrites at once; the reference decoder's pictures of the packets are
TH_ENCCTL_THIP_GET_RECON's; the quality statistics are a caller-side sum; with w = 0 every packet is the parent's."""
import numpy as np
import pytest

from tests import enc_cut_ref as CR
from tests import enc_ref
from tests import enc_rdq_ref as Q
from tests import enc_skip_ref as S
from tests import refcmp

pytestmark = pytest.mark.gpu

FIELDS = ("weight", "measured", "zeroed", "lowered", "emptied", "rate_before", "rate_after", "dist_before", "dist_after", "lam")


def _encode(w, h, fmt, quality, frames, rdq=3, skip=False, delta=0, k=0, modes=True, rd=False, kf=64, recon=False, device_input=False,
            quality_stats=False, **kw):
    """Headers, and per packet a dict: pkt, rdq, pack, cut, key, rate (bitrate mode), recon and quality (when asked for)."""
    from theora_amd.encoder import Encoder
    inter = kf != 1
    e = Encoder(w, h, fmt, quality, inter=inter, keyframe_interval=kf if inter else None, all_modes=modes and inter, block_qi=delta,
                masking=k, rd_modes=rd, rd_skip=skip, rd_quant=rdq, **kw)
    if quality_stats:
        e.set_quality_stats(("sse",))
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if device_input:
            import torch
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                t = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr]
                e.encode(t, stream=side)
                for a in t:
                    a.fill_(0x33)   # the caller's planes are its own again as soon as the call returns, on its stream
        else:
            e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], rdq=e.rd_quant_stats(), pack=e.pack_stats(), cut=e.cut_stats(),
                            key=e.inter_stats()["key"] if inter else 1, rate=e.rate_stats() if kw.get("bitrate") else None,
                            recon=e.recon() if recon and inter else None, quality=e.quality_stats() if quality_stats else None))
    e.close()
    return hdr, out


def _same_stats(got, want):
    assert {n: got[n] for n in FIELDS} == want, (got, want)
    assert got["rdq_ms"] > 0 if want["measured"] else got["rdq_ms"] == 0


def _compare(out, ref, frames, q):
    assert len(out) == len(frames)
    for f, fr in enumerate(frames):
        want = ref.frame(fr, q)
        g = out[f]
        _same_stats(g["rdq"], want["rdq"])
        assert g["pkt"] == want["packet"], (f, len(g["pkt"]), len(want["packet"]))
        if g["recon"] is not None:
            for p in range(3):
                assert np.array_equal(g["recon"][p], ref.recon[p]), (f, p)


def _run_case(case, **kw):
    kind, w, h, fmt, q, nf, kf, modes, delta, k, rd, skip, cw = case
    return _encode(w, h, fmt, q, Q.case_frames(case), rdq=cw, skip=skip, delta=delta, k=k, modes=modes, rd=rd, kf=kf, **kw)


@pytest.mark.parametrize("pack", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", Q.PACKET_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_rdq_packets_equal_the_restatement(hip, case, pack):
    frames = Q.case_frames(case)
    hdr, out = _run_case(case, recon=True, device_pack=pack)
    ref = Q.case_encoder(case, enc_ref.SetupParams(hdr[2]))
    try:
        _compare(out, ref, frames, case[4])
    finally:
        ref.close()
    assert all(g["rdq"]["measured"] == 1 and sum(g["rdq"]["zeroed"]) > 0 for g in out)
    assert sum(sum(g["rdq"]["lowered"]) for g in out) > 0
    if pack:
        assert all(g["pack"]["device"] == 1 for g in out)


@pytest.mark.parametrize("case", [Q.PACKET_CASES[1], Q.PACKET_CASES[3], Q.PACKET_CASES[4]], ids=lambda c: "-".join(str(v) for v in c))
def test_the_reference_decoder_reaches_the_encoders_reconstruction(hip, case):
    from oracle import ref
    refcmp.need_ref()
    hdr, out = _run_case(case, recon=True)
    dec = ref.RefDecoder(hdr)
    try:
        for n, g in enumerate(out):
            assert dec.packetin(g["pkt"])[0] == 0, n
            pic = dec.ycbcr_out()
            if g["recon"] is not None:
                for p in range(3):
                    assert np.array_equal(np.asarray(pic[p]), g["recon"][p]), (n, p)
    finally:
        dec.close()


def test_bitrate_mode_equals_the_restatement(hip):
    """The probe and the controller are unchanged: the qi sequence, the controller's record and the packets are those of the rate
    restatement around the rule's encoder."""
    w, h, fmt, bitrate = 96, 64, 0, 60000
    frames = S.clip("static", w, h, fmt, 4, seed=8)
    hdr, out = _encode(w, h, fmt, 32, frames, rdq=5, skip=True, bitrate=bitrate)
    rs = Q.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, kf_interval=64, w=5)
    want = []
    try:
        for fr in frames:
            want.extend(rs.frame(fr))
    finally:
        rs.close()
    assert len(out) == len(want)
    for n, (g, (wpkt, rec)) in enumerate(zip(out, want)):
        for name, v in rec.items():
            assert g["rate"][name] == v, (n, name, g["rate"][name], v)
        assert g["pkt"] == wpkt, n
        assert g["rdq"]["measured"] == int(bool(wpkt))
    assert sum(sum(g["rdq"]["zeroed"]) for g in out) > 0


def test_automatic_key_frames_equal_the_restatement(hip):
    w, h, fmt, q = 96, 64, 0, 32
    frames = CR.scene(w, h, fmt, 4, 2)
    hdr, out = _encode(w, h, fmt, q, frames, rdq=3, auto_keyframes=CR.RECOMMENDED)
    ref = Q.CutRdqEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6, skip=False, w=3)
    ref.t = CR.RECOMMENDED
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, q)
            _same_stats(out[f]["rdq"], want["rdq"])
            assert out[f]["pkt"] == want["packet"], f
            assert out[f]["cut"]["cut"] == want["cut"]["cut"] == int(f == 2)
    finally:
        ref.close()


def test_device_input_overwritten_at_once_and_quality_statistics(hip):
    """The kernel reads the source a second time: planes the caller overwrites on its own stream right after the call still give the
    host input's packets; and the quality statistics are the squared error of the reconstruction against the source."""
    case = Q.PACKET_CASES[6]
    frames = Q.case_frames(case)
    hdr, host = _run_case(case, recon=True, quality_stats=True)
    hdr2, dev = _run_case(case, device_input=True)
    assert hdr == hdr2 and [g["pkt"] for g in host] == [g["pkt"] for g in dev]
    assert [{n: g["rdq"][n] for n in FIELDS} for g in host] == [{n: g["rdq"][n] for n in FIELDS} for g in dev]
    for g, fr in zip(host, frames):
        assert g["quality"]["measured"] == 1
        for p in range(3):
            d = np.asarray(fr[p], np.int64) - np.asarray(g["recon"][p], np.int64)
            assert g["quality"]["sse"][p] == int((d * d).sum()), p


def test_weight_zero_is_the_parent(hip):
    """w = 0: SkipEncoder's packets (the stream before this switch existed), and the statistics of a frame not treated."""
    case = Q.PACKET_CASES[3]
    frames = Q.case_frames(case)
    hdr, off = _run_case(case[:12] + (0,))
    ref = Q.case_encoder(case, enc_ref.SetupParams(hdr[2]), w=0)
    try:
        for f, fr in enumerate(frames):
            assert off[f]["pkt"] == ref.frame(fr, case[4])["packet"], f
    finally:
        ref.close()
    zero = dict(weight=0, measured=0, zeroed=[0] * 3, lowered=[0] * 3, emptied=0, rate_before=0, rate_after=0, dist_before=0,
                dist_after=0, lam=0, rdq_ms=0.0)
    assert all(g["rdq"] == zero for g in off)


def test_rd_quant_only_before_the_first_frame_and_a_zero_byte_packet(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_RD_QUANT, Encoder
    frames = S.clip("pan", 64, 48, 0, 2)
    e = Encoder(64, 48, 0, 30, inter=True, rd_skip=True, rd_quant=3)
    e.header_packets()
    e.encode(frames[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_RD_QUANT, 0)[0] == -10
    assert e.packetout(False) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_RD_QUANT, 5)[0] == -10
    assert e.rd_quant_stats()["weight"] == 3 and e.rd_quant_stats()["measured"] == 1
    e.encode([np.ascontiguousarray(a) for a in e.recon()])   # the frame IS the reconstruction: nothing is coded
    r = e.packetout(True)
    st = e.rd_quant_stats()
    assert r[0] == b"" and st["measured"] == 0 and st["weight"] == 3 and st["rdq_ms"] == 0.0 and st["rate_before"] == 0
    e.close()
