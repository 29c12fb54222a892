"""th_encode_* under a caller's quantisation parameters (TH_ENCCTL_SET_QUANT_PARAMS) on the GPU.  Every kernel that reads a step --
the intra and inter block kernels, the block-qi choice, the rate-distortion modes, skip and level decisions, the rate probe -- runs
under parameters unlike the built-in ones (tests/enc_quant_ref.py: `ranges`, three ranges over four matrices for each of the six
tables; `saw`, scales that rise and fall with qi; `shared`, one matrix for everything), and every packet equals the existing
restatement built from the stream's own setup header, with the host packer and with the device packetiser.  The reconstruction is
this library's decoder's picture of the packets, and the reference decoder's.  In bitrate mode and in both passes of two-pass under
`saw` the probe's E[q] equals tests/enc_rate_ref.py's at all 64 q, and the chosen qi is the restated controller's.

Sizes: 64 x 48 and 176 x 144, 4:2:0, one 4:4:4 case; at most 6 frames: the smallest at which every plane has interior, border and
multi-super-block fragments."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_2pass_ref as TP
from tests import enc_inter_ref as R
from tests import enc_quant_ref as QR
from tests import enc_rdq_ref as Q
from tests import enc_ref, refcmp
from tests import enc_skip_ref as S

pytestmark = pytest.mark.gpu

# name: (clip, w, h, fmt, quality, frames, key-frame interval, eight modes, block-qi delta, masking, RD modes, skip, level weight, bitrate)
MODES = {
    "key-only": ("pan", 176, 144, 0, 40, 2, 1, False, 0, 0, False, False, 0, None),
    "five-modes": ("pan", 176, 144, 0, 32, 3, 64, False, 0, 0, False, False, 0, None),
    "eight-modes": ("pan", 64, 48, 3, 32, 4, 64, True, 0, 0, False, False, 0, None),
    "block-qi-masking": ("pan", 64, 48, 0, 32, 3, 64, False, 8, 4, False, False, 0, None),
    "rd-modes": ("pan", 64, 48, 0, 24, 4, 64, True, 0, 0, True, False, 0, None),
    "skip": ("static", 64, 48, 0, 40, 4, 64, False, 0, 0, False, True, 0, None),
    "level-choice-16": ("pan", 64, 48, 0, 32, 3, 64, True, 8, 0, False, False, 16, None),
    "bitrate": ("pan", 64, 48, 0, 32, 5, 64, True, 0, 0, False, False, 0, 60000),
}
FAMILIES = ("ranges", "saw", "shared")


@pytest.fixture(scope="module")
def fams():
    return QR.families()


def _frames(mode):
    kind, w, h, fmt = MODES[mode][:4]
    return S.clip(kind, w, h, fmt, MODES[mode][5], seed=MODES[mode][4])


def _encode(mode, quant, pack):
    """-> (headers, per packet dict(pkt, recon, stats, pack, rate))."""
    from theora_amd.encoder import Encoder
    kind, w, h, fmt, q, nf, kf, modes, delta, k, rd, skip, cw, bitrate = MODES[mode]
    inter = kf != 1
    e = Encoder(w, h, fmt, q, inter=inter, keyframe_interval=kf if inter else None, all_modes=modes and inter, block_qi=delta,
                masking=k, rd_modes=rd, rd_skip=skip, rd_quant=cw, bitrate=bitrate, device_pack=pack, quant=quant)
    hdr = e.header_packets()
    frames, out = _frames(mode), []
    for f, fr in enumerate(frames):
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], recon=e.recon() if inter else None, stats=e.stats(), pack=e.pack_stats(), rate=e.rate_stats() if bitrate else None))
    e.close()
    return hdr, out


def _restated(mode, hdr):
    """The existing restatement of the mode, every table read from the stream's setup header -> [(packet, record or None,
    the restatement's reconstruction after the packet)]."""
    kind, w, h, fmt, q, nf, kf, modes, delta, k, rd, skip, cw, bitrate = MODES[mode]
    setup, pic = enc_ref.SetupParams(hdr[2]), (0, 0, w, h)
    if bitrate:
        rs = Q.RateStream(w, h, fmt, pic, setup, bitrate, kf_interval=kf, delta=delta, k=k, modes=modes, rd=rd, skip=skip, w=cw)
        try:
            return [x + (rs.enc.recon,) for fr in _frames(mode) for x in rs.frame(fr)]
        finally:
            rs.close()
    ref = Q.RdqEncoder(w, h, fmt, pic, setup, kf, 6, delta, k, modes, rd, skip, cw)
    try:
        return [(ref.frame(fr, q)["packet"], None, ref.recon) for fr in _frames(mode)]
    finally:
        ref.close()


def _decoded(hdr, packets, recons, what):
    """recons are this library's decoder's pictures of the packets, and the reference decoder's where it is present."""
    from oracle import ref
    from theora_amd.decoder import Decoder
    dec, rd = Decoder(hdr), ref.RefDecoder(hdr) if ref.available() else None
    try:
        for n, (pkt, want) in enumerate(zip(packets, recons)):
            assert dec.packetin(pkt)[0] >= 0, (what, n)
            assert not refcmp.diff_planes(dec.ycbcr_out(), want), (what, n)
            if rd:
                assert rd.packetin(pkt)[0] >= 0, (what, n)
                assert not refcmp.diff_planes(rd.ycbcr_out(), want), (what, n)
    finally:
        dec.close()
        if rd:
            rd.close()


def test_fails_without_the_feature(hip, fams):
    """Request 2 with a th_quant_info answers 0 and request 0x7229 answers 0: both were TH_EIMPL before."""
    from theora_amd import encoder as E
    e = E.Encoder(64, 48, 0, 32)
    s = fams["saw"].quant_info().struct()
    assert e._L.th_encode_ctl(e._enc, 2, C.byref(s), C.sizeof(s)) == 0
    g = E.QuantInfoStruct()
    assert e._L.th_encode_ctl(e._enc, 0x7229, C.byref(g), C.sizeof(g)) == 0
    e.close()


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("mode", list(MODES))
def test_packets_equal_the_restatement(hip, fams, mode, name):
    """Host packer and device packetiser: byte for byte the restatement's packets; the reconstruction is the decoders' picture."""
    p = fams[name]
    hdr, host = _encode(mode, p.quant_info(), False)
    hdr2, dev = _encode(mode, p.quant_info(), True)
    assert hdr == hdr2 and p.same(QR.from_setup(enc_ref.SetupParams(hdr[2])).quant_info())
    want = _restated(mode, hdr)
    assert len(host) == len(dev) == len(want)
    for n, (a, b, (w, rec, recon)) in enumerate(zip(host, dev, want)):
        assert a["pkt"] == w, (mode, name, n, "host packer", len(a["pkt"]), len(w))
        assert b["pkt"] == w, (mode, name, n, "device packetiser", len(b["pkt"]), len(w))
        if w:
            assert a["pack"]["device"] == 0 and b["pack"]["device"] == 1
        # TH_ENCCTL_THIP_GET_RECON is the restatement's reconstruction.  (A key-only encoder keeps none -- the request answers
        # TH_EINVAL without inter frames -- so for that stack the decoders' pictures below are held against the restatement's.)
        for got in (a["recon"], b["recon"]):
            assert got is None or not refcmp.diff_planes(got, recon), (mode, name, n)
        if rec is not None and not rec.get("duplicate"):
            for got in (a["rate"], b["rate"]):
                assert got["probe"] == rec["probe"] and got["qi"] == rec["qi"] and got["key"] == rec["key"], (mode, name, n)
    assert any(len(x[0]) for x in want)
    assert all((a["recon"] is None) == (mode == "key-only") for a in host)
    _decoded(hdr, [a["pkt"] for a in host], [x[2] if a["recon"] is None else a["recon"] for a, x in zip(host, want)], (mode, name))


def test_probe_under_saw_bitrate_mode(hip, fams):
    """Bitrate mode, 176 x 144 five-mode inter frames under `saw`: thip_enc_rate_stats.probe equals tests/enc_rate_ref.py's Probe
    built from the header at all 64 q, on key and inter frames -- E[q] is not monotone in q, and the qi chosen is the restated
    controller's."""
    from tests import enc_rate_ref as RR
    from theora_amd.encoder import Encoder
    w, h, fmt = 176, 144, 0
    frames = R.sequence("pan", w, h, fmt, 4, seed=7)
    e = Encoder(w, h, fmt, 32, inter=True, keyframe_interval=3, bitrate=150000, quant=fams["saw"].quant_info())
    hdr = e.header_packets()
    rs = RR.RateStream(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 150000, inter=True, kf_interval=3)
    try:
        keys = 0
        for f, fr in enumerate(frames):
            e.encode(fr)
            pkt = e.packetout(f == len(frames) - 1)[0]
            got = e.rate_stats()
            (wpkt, rec), = rs.frame(fr)
            assert got["probe"] == rec["probe"] and (got["qi"], got["key"]) == (rec["qi"], rec["key"]), f
            assert pkt == wpkt, f
            E = np.array(rec["probe"])
            assert (np.diff(E) < 0).any() and (np.diff(E) > 0).any(), f      # up and down with q
            keys += rec["key"]
        assert 0 < keys < len(frames)
    finally:
        rs.close()
        e.close()


def test_two_pass_under_saw(hip, fams):
    """Both passes under `saw` (the pass file does not carry the quantisers: both passes are given the same ones): the recorded
    curves and the second pass's choices and packets equal the restatement's."""
    from tests.test_gpu_encoder_2pass import _first, _second
    w, h, fmt, n, kf, bitrate = 64, 48, 0, 6, 4, 60000
    quant = fams["saw"].quant_info()
    frames = R.sequence("pan", w, h, fmt, n, seed=13)
    kw = dict(inter=True, keyframe_interval=kf, quant=quant)
    hdr, got1, data, _ = _first(w, h, fmt, frames, quality=40, **kw)
    setup = enc_ref.SetupParams(hdr[2])
    p1 = TP.Pass1(w, h, fmt, (0, 0, w, h), setup, quality=40, bitrate=None, inter=True, kf_interval=kf)
    try:
        want1 = [x for fr in frames for x in p1.frame(fr, 0)]
        assert [g[0] for g in got1] == [x[0] for x in want1]
        assert data == p1.file()
    finally:
        p1.close()
    hdr2, got2 = _second(w, h, fmt, frames, data, bitrate, **kw)
    assert hdr2[2] == hdr[2]                # (the info header differs: it carries the second pass's bitrate)
    p2 = TP.Pass2(w, h, fmt, (0, 0, w, h), setup, bitrate, data, inter=True)
    try:
        want2 = [x for fr in frames for x in p2.frame(fr, 0)]
    finally:
        p2.close()
    assert len(got2) == len(want2)
    for k, ((pkt, gp, rate, tp), (wpkt, st)) in enumerate(zip(got2, want2)):
        assert (rate["qi"], rate["key"], rate["probe"], rate["actual"]) == (st["qi"], st["key"], st["probe"], st["actual"]), k
        assert (tp["qi"], tp["fresh"], tp["recorded"]) == (st["qi"], st["probe"], st["recorded"]), k
        assert pkt == wpkt, k


@pytest.mark.parametrize("name", ["edge-low", "edge-high"])
def test_edge_parameters(hip, fams, name):
    """63 ranges of size 1, scales of 1 and 65535, limits all 0 and all 127: the header is the restatement's, and a key frame and
    an inter frame at qi 0, 31 and 63 are byte-equal to the restatement and decodable."""
    from theora_amd.encoder import Encoder
    p = fams[name]
    w, h, fmt = 64, 48, 0
    for qi in (0, 31, 63):
        frames = R.sequence("pan", w, h, fmt, 2, seed=qi)
        e = Encoder(w, h, fmt, qi, inter=True, quant=p.quant_info())
        hdr = e.header_packets()
        assert p.same(QR.from_setup(enc_ref.SetupParams(hdr[2])).quant_info())
        ref = R.InterEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
        pkts, recons = [], []
        try:
            for f, fr in enumerate(frames):
                e.encode(fr)
                pkts.append(e.packetout(f == 1)[0])
                recons.append(e.recon())
                assert pkts[-1] == ref.frame(fr, qi)["packet"], (name, qi, f)
                assert not refcmp.diff_planes(recons[-1], ref.recon), (name, qi, f)
        finally:
            ref.close()
            e.close()
        _decoded(hdr, pkts, recons, (name, qi))


def test_loop_filter_limits(hip, fams):
    """The loop filter with limit 127 and with limit 0 at every qi: the reconstruction is the restatement's oracle picture, and the
    two differ from each other (the limit reaches the filter)."""
    from theora_amd.encoder import Encoder
    w, h, fmt, qi = 64, 48, 0, 10
    frames = R.sequence("pan", w, h, fmt, 2, seed=2)
    first = {}
    for limit in (0, 127):
        p = fams["ranges"].copy()
        p.lf = [limit] * 64
        e = Encoder(w, h, fmt, qi, inter=True, quant=p.quant_info())
        hdr = e.header_packets()
        ref = R.InterEncoder(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
        pkts, recons = [], []
        try:
            for f, fr in enumerate(frames):
                e.encode(fr)
                pkts.append(e.packetout(f == 1)[0])
                recons.append(e.recon())
                assert pkts[-1] == ref.frame(fr, qi)["packet"], (limit, f)
                assert not refcmp.diff_planes(recons[-1], ref.recon), (limit, f)
        finally:
            ref.close()
            e.close()
        _decoded(hdr, pkts, recons, limit)
        first[limit] = recons[0]
    assert refcmp.diff_planes(first[0], first[127])


def test_encoder_example_quant_from(hip, fams, tmp_path):
    """examples/encoder_example_hip.c --quant-from FILE.ogv codes with the quantisers of FILE's setup header: the stream of the
    Python encoder given the same parameters; a file without a Theora setup header is refused."""
    import subprocess
    from tests.test_gpu_encoder import _compile, _y4m
    from theora_amd.decoder import ogg_packets
    from theora_amd.encoder import Encoder, ogg_stream
    w, h, fmt, q = 64, 48, 0, 32
    frames = R.sequence("pan", w, h, fmt, 3, seed=1)
    src = Encoder(w, h, fmt, q, quant=fams["saw"].quant_info())
    (tmp_path / "other.ogv").write_bytes(ogg_stream(src.header_packets(), []))
    src.close()
    e = Encoder(w, h, fmt, q, inter=True, keyframe_interval=3, quant=fams["saw"].quant_info())
    hdr, want = e.header_packets(), []
    for f, fr in enumerate(frames):
        e.encode(fr)
        want.append(e.packetout(f == len(frames) - 1)[0])
    e.close()
    exe = _compile(tmp_path, "encoder_example_hip")
    (tmp_path / "in.y4m").write_bytes(_y4m(frames, w, h, "420jpeg"))
    args = [exe, "-q", str(q), "-k", "3", "-o", str(tmp_path / "out.ogv")]
    r = subprocess.run(args + ["--quant-from", str(tmp_path / "other.ogv"), str(tmp_path / "in.y4m")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    packets, (bad, gaps) = ogg_packets((tmp_path / "out.ogv").read_bytes())
    assert (bad, gaps) == (0, 0) and [p[1] for p in packets] == hdr + want
    r = subprocess.run(args + ["--quant-from", str(tmp_path / "in.y4m"), str(tmp_path / "in.y4m")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "setup header" in r.stderr
