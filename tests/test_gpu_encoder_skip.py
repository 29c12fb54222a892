"""th_encode_* with the skip decision on the GPU (TH_ENCCTL_THIP_SET_RD_SKIP): the packets, the skip statistics and the reconstruction
equal tests/enc_skip_ref.py's restatement byte for byte -- over enc_skip_ref.PACKET_CASES (the static clip and the pan at 64 x 48 and
176 x 144, the three pixel formats, five and eight modes, block qi, masking, the rate-distortion mode decision;
tests/test_encoder_skip_cpu.py asserts that none of them is vacuous) -- and so they do with the device packetiser, in bitrate mode and
with automatic key frames; the reference decoder's pictures of the packets are TH_ENCCTL_THIP_GET_RECON's; with the switch off every
packet is the parent's."""
import numpy as np
import pytest

from tests import enc_cut_ref as CR
from tests import enc_ref
from tests import enc_skip_ref as S
from tests import refcmp

pytestmark = pytest.mark.gpu

FIELDS = ("on", "measured", "skipped", "demoted", "lam")


def _encode(w, h, fmt, quality, frames, skip=True, delta=0, k=0, modes=True, rd=False, kf=64, recon=False, **kw):
    """Headers, and per packet a dict: pkt, skip, pack, cut, rate (bitrate mode), recon (when asked for)."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, quality, inter=True, keyframe_interval=kf, all_modes=modes, block_qi=delta, masking=k, rd_modes=rd,
                rd_skip=skip, **kw)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], skip=e.skip_stats(), pack=e.pack_stats(), cut=e.cut_stats(), key=e.inter_stats()["key"],
                            rate=e.rate_stats() if kw.get("bitrate") else None, recon=e.recon() if recon else None))
    e.close()
    return hdr, out


def _same_stats(got, want):
    assert {n: got[n] for n in FIELDS} == want, (got, want)
    assert got["skip_ms"] > 0 if want["measured"] else got["skip_ms"] == 0


def _compare(out, ref, frames, q):
    assert len(out) == len(frames)
    for f, fr in enumerate(frames):
        want = ref.frame(fr, q)
        g = out[f]
        _same_stats(g["skip"], want["skip"])
        assert g["pkt"] == want["packet"], (f, len(g["pkt"]), len(want["packet"]))
        if g["recon"] is not None:
            for p in range(3):
                assert np.array_equal(g["recon"][p], ref.recon[p]), (f, p)


@pytest.mark.parametrize("pack", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", S.PACKET_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_skip_packets_equal_the_restatement(hip, case, pack):
    kind, w, h, fmt, q, nf, modes, delta, k, rd = case
    frames = S.case_frames(case)
    hdr, out = _encode(w, h, fmt, q, frames, delta=delta, k=k, modes=modes, rd=rd, recon=True, device_pack=pack)
    ref = S.case_encoder(case, enc_ref.SetupParams(hdr[2]))
    try:
        _compare(out, ref, frames, q)
    finally:
        ref.close()
    assert out[0]["skip"]["measured"] == 0 and out[0]["skip"]["on"] == 1          # the key frame
    assert sum(sum(g["skip"]["skipped"]) for g in out) > 0 and sum(g["skip"]["demoted"] for g in out) > 0
    if pack:
        assert all(g["pack"]["device"] == 1 for g in out)


@pytest.mark.parametrize("case", [S.PACKET_CASES[1], S.PACKET_CASES[2], S.PACKET_CASES[4]], ids=lambda c: "-".join(str(v) for v in c))
def test_the_reference_decoder_reaches_the_encoders_reconstruction(hip, case):
    from oracle import ref
    refcmp.need_ref()
    kind, w, h, fmt, q, nf, modes, delta, k, rd = case
    hdr, out = _encode(w, h, fmt, q, S.case_frames(case), delta=delta, k=k, modes=modes, rd=rd, recon=True)
    dec = ref.RefDecoder(hdr)
    try:
        for n, g in enumerate(out):
            assert dec.packetin(g["pkt"])[0] == 0, n
            pic = dec.ycbcr_out()
            for p in range(3):
                assert np.array_equal(np.asarray(pic[p]), g["recon"][p]), (n, p)
    finally:
        dec.close()


def test_bitrate_mode_equals_the_restatement(hip):
    """The probe and the controller are unchanged: the qi sequence, the controller's record and the packets are those of the rate
    restatement around the rule's encoder."""
    w, h, fmt, bitrate = 96, 64, 0, 60000
    frames = S.clip("static", w, h, fmt, 4, seed=8)
    hdr, out = _encode(w, h, fmt, 32, frames, bitrate=bitrate)
    rs = S.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, kf_interval=64)
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
        assert g["skip"]["measured"] == int(bool(wpkt) and not rec["key"])
    assert sum(sum(g["skip"]["skipped"]) for g in out) > 0


def test_automatic_key_frames_equal_the_restatement(hip):
    w, h, fmt, q = 96, 64, 0, 32
    frames = CR.scene(w, h, fmt, 4, 2)
    hdr, out = _encode(w, h, fmt, q, frames, auto_keyframes=CR.RECOMMENDED)
    ref = S.CutSkipEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
    ref.t = CR.RECOMMENDED
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, q)
            _same_stats(out[f]["skip"], want["skip"])
            assert out[f]["pkt"] == want["packet"], f
            assert out[f]["cut"]["cut"] == want["cut"]["cut"] == int(f == 2)
    finally:
        ref.close()


def test_switch_off_and_a_static_scene(hip):
    """Off: the parent's packets, measured = 0.  On, a frame that IS the reconstruction becomes the zero-byte packet, whose statistics
    are those of a frame not decided."""
    case = S.PACKET_CASES[1]
    kind, w, h, fmt, q, nf, modes, delta, k, rd = case
    frames = S.case_frames(case)
    hdr, off = _encode(w, h, fmt, q, frames, skip=False, modes=modes)
    ref = S.case_encoder(case, enc_ref.SetupParams(hdr[2]), skip=False)
    try:
        for f, fr in enumerate(frames):
            assert off[f]["pkt"] == ref.frame(fr, q)["packet"], f
    finally:
        ref.close()
    assert all(g["skip"] == dict(on=0, measured=0, skipped=[0] * 3, demoted=0, lam=0, skip_ms=0.0) for g in off)
    hdr, first = _encode(w, h, fmt, q, frames[:1], modes=modes, recon=True)
    hdr, on = _encode(w, h, fmt, q, [frames[0], [np.ascontiguousarray(a) for a in first[0]["recon"]], frames[1]], modes=modes)
    assert on[1]["pkt"] == b"" and on[1]["skip"] == dict(on=1, measured=0, skipped=[0] * 3, demoted=0, lam=0, skip_ms=0.0)
    assert on[2]["pkt"] and on[2]["skip"]["measured"] == 1


def test_rd_skip_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_RD_SKIP, Encoder
    e = Encoder(64, 48, 0, 30, inter=True, rd_skip=True)
    e.header_packets()
    e.encode(S.clip("pan", 64, 48, 0, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_RD_SKIP, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_RD_SKIP, 1)[0] == -10
    assert e.skip_stats()["on"] == 1 and e.skip_stats()["measured"] == 0
    e.close()
