"""th_encode_* with the rate-distortion mode decision on the GPU (TH_ENCCTL_THIP_SET_RD_MODES): the packets, the mode statistics and
the rd statistics equal tests/enc_rd_ref.py's restatement byte for byte -- over enc_rd_ref.PACKET_CASES (sizes 64 x 48 to 176 x 144,
qualities 0 / 16 / 48 / 63, the three pixel formats; tests/test_encoder_rd_cpu.py asserts that every candidate wins among them) -- and
so they do composed with block qi, masking, bitrate mode, automatic key frames, the device packetiser, R'G'B' input and device input;
with the switch off, or on with five modes, every packet is the parent's."""
import numpy as np
import pytest

from tests import enc_cut_ref as CR
from tests import enc_inter_ref as IR
from tests import enc_modes_ref as M
from tests import enc_rd_ref as RD
from tests import enc_ref
from tests.test_gpu_encoder_mask import _rgb_frames

pytestmark = pytest.mark.gpu

RD_FIELDS = ("on", "measured", "huff", "lam")


def _encode(w, h, fmt, quality, frames, rd=True, delta=0, k=0, pic=None, modes=True, kf=64, dev=False, rgb=False, recon=False, **kw):
    """Headers, and per packet a dict: pkt, rd, modes, mask, cut, pack, rate (bitrate mode), recon (when asked for)."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, inter=True, keyframe_interval=kf, all_modes=modes, block_qi=delta, masking=k, rd_modes=rd, **kw)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        if rgb:
            e.encode_rgb(fr, "rgb")
        elif dev:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], rd=e.rd_stats(), modes=e.mode_stats(), mask=e.mask_stats(), cut=e.cut_stats(), pack=e.pack_stats(),
                            rate=e.rate_stats() if kw.get("bitrate") else None, recon=e.recon() if recon else None))
    e.close()
    return hdr, out


def _same_rd(got, want):
    assert {n: got[n] for n in RD_FIELDS} == want, (got, want)
    assert got["rd_ms"] > 0 if want["measured"] else got["rd_ms"] == 0


def _compare(out, ref, frames, q):
    wins = np.zeros(6, int)
    assert len(out) == len(frames)
    for f, fr in enumerate(frames):
        want = ref.frame(fr, q)
        g = out[f]
        _same_rd(g["rd"], want["rd"])
        assert g["pkt"] == want["packet"], (f, len(g["pkt"]), len(want["packet"]))
        assert list(g["modes"]["modes"].values()) == list(want["modes8"]) and g["modes"]["vectors"] == want["vectors"], f
        if g["recon"] is not None:   # the decoder's picture of the packets so far
            for p in range(3):
                assert np.array_equal(g["recon"][p], ref.recon[p]), (f, p)
        if want["rd"]["measured"]:
            wins += np.bincount(want["decision"]["cand"], minlength=6)
    return wins


@pytest.mark.parametrize("case", RD.PACKET_CASES, ids=lambda c: "%s-%dx%d-f%d-q%d" % c[:5])
def test_rd_packets_equal_the_restatement(hip, case):
    kind, w, h, fmt, q, nf = case
    frames = RD.case_frames(case)
    hdr, out = _encode(w, h, fmt, q, frames, recon=True)
    ref = RD.RdEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
    try:
        wins = _compare(out, ref, frames, q)
    finally:
        ref.close()
    assert wins.sum() > 0
    assert out[0]["rd"]["measured"] == 0 and out[0]["rd"]["on"] == 1          # the key frame
    assert out[1]["rd"]["huff"] == [5, 5, 5, 5]                               # before an inter packet exists
    assert out[1]["rd"]["lam"] == RD.rd_lambda(enc_ref.SetupParams(hdr[2]).qmat(1, 0, q)[enc_ref.ZIGZAG][1])


@pytest.mark.parametrize("cross", ["block_qi", "block_qi_masking", "device_pack", "device_input", "pic_region"])
def test_compositions_equal_the_restatement(hip, cross):
    w, h, fmt, q = 96, 64, 0, 32
    delta, k = (8, 0) if cross == "block_qi" else (8, 4) if cross == "block_qi_masking" else (0, 0)
    pic = (5, 3, 83, 55) if cross == "pic_region" else None
    frames = M.sequence("uncover", w, h, fmt, 4, seed=12)
    if pic:
        frames = [[np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in
                   zip(fr, (enc_ref.chroma_region(pic, fmt, p) for p in range(3)))] for fr in frames]
    hdr, out = _encode(w, h, fmt, q, frames, delta=delta, k=k, pic=pic, dev=cross == "device_input",
                       **(dict(device_pack=True) if cross == "device_pack" else {}))
    ref = RD.RdEncoder(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6, delta, k)
    try:
        wins = _compare(out, ref, frames, q)
    finally:
        ref.close()
    assert (wins > 0).sum() >= 2, wins
    if cross == "device_pack":
        assert all(g["pack"]["device"] == 1 for g in out)
    if k:
        assert all(g["mask"]["measured"] == 1 for g in out)
    assert [g["rd"]["huff"] for g in out[2:]] != [[5] * 4] * len(out[2:])   # the tables follow the previous inter packet


def test_rgb_input_equals_the_restatement(hip):
    from tests import picture_in_ref
    w, h, fmt, q, pic = 96, 64, 0, 32, (5, 3, 83, 55)
    images = _rgb_frames(pic[2], pic[3], 3, 2)
    frames = [picture_in_ref.picture_in(im, fmt, "rgb", pic[0], pic[1]) for im in images]
    hdr, out = _encode(w, h, fmt, q, images, pic=pic, rgb=True)
    ref = RD.RdEncoder(w, h, fmt, pic, enc_ref.SetupParams(hdr[2]), 64, 6)
    try:
        _compare(out, ref, frames, q)
    finally:
        ref.close()


def test_automatic_key_frames_equal_the_restatement(hip):
    w, h, fmt, q = 96, 64, 0, 32
    frames = CR.scene(w, h, fmt, 4, 2)
    hdr, out = _encode(w, h, fmt, q, frames, auto_keyframes=CR.RECOMMENDED)
    ref = RD.CutRdEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
    ref.t = CR.RECOMMENDED
    try:
        for f, fr in enumerate(frames):
            want = ref.frame(fr, q)
            _same_rd(out[f]["rd"], want["rd"])
            assert out[f]["pkt"] == want["packet"], f
            assert out[f]["cut"]["cut"] == want["cut"]["cut"] == int(f == 2)
            assert out[f]["rd"]["measured"] == int(f in (1, 3))   # a cut frame is a key frame: not decided by the rule
    finally:
        ref.close()


def test_bitrate_mode_equals_the_restatement(hip):
    """The probe and the controller are unchanged: the qi sequence, the controller's record and the packets are those of the rate
    restatement around the rule's encoder."""
    w, h, fmt, bitrate = 96, 64, 0, 150000
    frames = M.sequence("uncover", w, h, fmt, 4, seed=8)
    hdr, out = _encode(w, h, fmt, 32, frames, bitrate=bitrate)
    rs = RD.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, kf_interval=64)
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
        assert g["rd"]["measured"] == int(bool(wpkt) and not rec["key"])


def test_switch_off_and_five_modes(hip):
    """Off: the eight-mode encoder's packets, measured = 0.  On with five modes: no effect."""
    kind, w, h, fmt, q, nf = RD.PACKET_CASES[0]   # (a case whose modes differ from the cascade's: tests/test_encoder_rd_cpu.py)
    frames = RD.case_frames(RD.PACKET_CASES[0])
    setup = None
    for modes, Ref in ((True, M.ModesEncoder), (False, IR.InterEncoder)):
        off = _encode(w, h, fmt, q, frames, rd=False, modes=modes)
        on = _encode(w, h, fmt, q, frames, rd=True, modes=modes)
        setup = enc_ref.SetupParams(off[0][2])
        ref = Ref(w, h, fmt, (0, 0, w, h), setup, 64, 6)
        try:
            for f, fr in enumerate(frames):
                assert off[1][f]["pkt"] == ref.frame(fr, q)["packet"], (modes, f)
        finally:
            ref.close()
        assert all(g["rd"] == dict(on=0, measured=0, huff=[0] * 4, lam=0, rd_ms=0.0) for g in off[1])
        if modes:
            assert [g["pkt"] for g in on[1]] != [g["pkt"] for g in off[1]]      # the rule does change them
            assert [g["rd"]["measured"] for g in on[1]] == [0, 1, 1, 1]
        else:
            assert [g["pkt"] for g in on[1]] == [g["pkt"] for g in off[1]]
            assert all(g["rd"] == dict(on=1, measured=0, huff=[0] * 4, lam=0, rd_ms=0.0) for g in on[1])


def test_rd_modes_only_before_the_first_frame(hip):
    from theora_amd.encoder import TH_ENCCTL_THIP_SET_RD_MODES, Encoder
    e = Encoder(64, 48, 0, 30, inter=True, all_modes=True, rd_modes=True)
    e.header_packets()
    e.encode(M.sequence("pan", 64, 48, 0, 1)[0])
    assert e.ctl(TH_ENCCTL_THIP_SET_RD_MODES, 0)[0] == -10
    assert e.packetout(True) is not None
    assert e.ctl(TH_ENCCTL_THIP_SET_RD_MODES, 1)[0] == -10
    assert e.rd_stats()["on"] == 1 and e.rd_stats()["measured"] == 0
    e.close()
