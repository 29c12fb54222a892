"""th_encode_* with custom and trained Huffman codes (TH_ENCCTL_SET_HUFFMAN_CODES, TH_ENCCTL_THIP_GET_TOKEN_HIST, thip_huff_train) on the
GPU.  Every kernel that reads code lengths -- the block-qi choice, the rate-distortion candidates, the skip and level decisions, the
rate probe, both packers -- runs under codes that are nothing like the built-in ones (the comb: lengths 1..31; the built-in lengths
moved between tokens; trained codes), and every packet equals the existing restatement built from the stream's own setup header.
The histogram equals tests/enc_huff_ref.py's in both packers; a 43-bit token goes through the packetiser; training is lossless, and
saves exactly the bits the trainer says; the reference encoder's streams under deep trees decode here as in the reference decoder.

Sizes: 64 x 48, and 80 x 64 with the picture region at odd offsets; 4:2:0 and 4:4:4; 2 to 5 frames."""
import ctypes as C

import numpy as np
import pytest

from tests import enc_huff_ref as HR
from tests import enc_inter_ref as R
from tests import enc_rdq_ref as Q
from tests import enc_ref, refcmp
from tests import enc_skip_ref as S
from tests import packref as P

pytestmark = pytest.mark.gpu

ODD = (3, 5, 71, 53)   # the picture region of the 80 x 64 cases

# name: (clip, w, h, fmt, pic, quality, frames, key-frame interval, eight modes, block-qi delta, masking, RD modes, skip, level weight,
# bitrate)
MODES = {
    "key-only": ("pan", 64, 48, 0, None, 40, 2, 1, False, 0, 0, False, False, 0, None),
    "five-modes": ("pan", 80, 64, 0, ODD, 32, 4, 64, False, 0, 0, False, False, 0, None),
    "eight-modes": ("pan", 64, 48, 3, None, 32, 4, 64, True, 0, 0, False, False, 0, None),
    "block-qi-masking": ("pan", 80, 64, 3, ODD, 32, 3, 64, False, 8, 4, False, False, 0, None),
    "rd-modes": ("pan", 64, 48, 0, None, 24, 4, 64, True, 0, 0, True, False, 0, None),
    "skip": ("static", 64, 48, 0, None, 40, 4, 64, False, 0, 0, False, True, 0, None),
    "level-choice-16": ("pan", 80, 64, 0, ODD, 32, 3, 64, True, 8, 0, False, False, 16, None),
    "bitrate": ("pan", 64, 48, 0, None, 32, 5, 64, True, 0, 0, False, False, 0, 60000),
}
CODE_SETS = ("comb", "rotated", "trained")


@pytest.fixture(scope="module")
def code_sets():
    """The three foreign code sets; `trained` from the restatements' histograms of a key and an inter clip (no GPU)."""
    from theora_amd.encoder import Encoder, train_huffman
    e = Encoder(64, 48, 0, 32)
    builtin = e.huffman_codes()
    setup = enc_ref.SetupParams(e.header_packets()[2])
    e.close()
    hists = [HR.hist_of_words(enc_ref.encode_frame(enc_ref.picture("natural", 64, 48, 0, seed=s), 64, 48, 0, (0, 0, 64, 48), q, setup)["words"])
             for s, q in ((1, 24), (2, 40), (3, 56))]
    enc = R.InterEncoder(64, 48, 0, (0, 0, 64, 48), setup, 64, 6)
    for fr in R.sequence("pan", 64, 48, 0, 4, seed=2):
        r = enc.frame(fr, 32)
        if "words" in r:   # (the inter frames; the key frames' tokens are above)
            hists.append(HR.hist_of_words(r["words"]))
    enc.close()
    trained, st = train_huffman(hists)
    assert st["bits_end"] < st["bits_start"]
    return dict(builtin=builtin, comb=HR.comb_codes(HR.comb_order), rotated=HR.rotated_codes(builtin), trained=trained)


def _frames(mode):
    kind, w, h, fmt = MODES[mode][:4]
    return S.clip(kind, w, h, fmt, MODES[mode][6], seed=MODES[mode][5])


def _encoder(mode, codes, pack):
    from theora_amd.encoder import Encoder
    kind, w, h, fmt, pic, q, nf, kf, modes, delta, k, rd, skip, cw, bitrate = MODES[mode]
    inter = kf != 1
    return Encoder(w, h, fmt, q, pic=pic, inter=inter, keyframe_interval=kf if inter else None, all_modes=modes and inter, block_qi=delta,
                   masking=k, rd_modes=rd, rd_skip=skip, rd_quant=cw, bitrate=bitrate, device_pack=pack, huffman=codes)


def _encode(mode, codes, pack):
    """-> (headers, per packet dict(pkt, hist, stats, pack))."""
    e = _encoder(mode, codes, pack)
    hdr = e.header_packets()
    frames, out = _frames(mode), []
    for f, fr in enumerate(frames):
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append(dict(pkt=r[0], hist=e.token_hist(), stats=e.stats(), pack=e.pack_stats()))
    e.close()
    return hdr, out


def _restated(mode, hdr):
    """The packets of the existing restatement of the mode, its codes read from the stream's setup header."""
    kind, w, h, fmt, pic, q, nf, kf, modes, delta, k, rd, skip, cw, bitrate = MODES[mode]
    setup, pic = enc_ref.SetupParams(hdr[2]), pic or (0, 0, w, h)
    if bitrate:
        rs = Q.RateStream(w, h, fmt, pic, setup, bitrate, kf_interval=kf, delta=delta, k=k, modes=modes, rd=rd, skip=skip, w=cw)
        try:
            return [pkt for fr in _frames(mode) for pkt, _ in rs.frame(fr)]
        finally:
            rs.close()
    ref = Q.RdqEncoder(w, h, fmt, pic, setup, kf, 6, delta, k, modes, rd, skip, cw)
    try:
        return [ref.frame(fr, q)["packet"] for fr in _frames(mode)]
    finally:
        ref.close()


def test_fails_without_the_feature(hip, code_sets):
    """Request 0 with a full-size buffer answers 0 and request 0x7227 answers 0: both were TH_EIMPL before."""
    from theora_amd import encoder as E
    e = E.Encoder(64, 48, 0, 32)
    buf = E._huff_codes_in(code_sets["comb"])
    assert e._L.th_encode_ctl(e._enc, 0, C.byref(buf), C.sizeof(buf)) == 0
    h = E.TokenHist()
    assert e._L.th_encode_ctl(e._enc, 0x7227, C.byref(h), C.sizeof(h)) == 0
    e.close()


@pytest.mark.parametrize("name", CODE_SETS)
@pytest.mark.parametrize("mode", list(MODES))
def test_packets_equal_the_restatement(hip, code_sets, mode, name):
    """Host packer and device packetiser, byte for byte the restatement's packets, under foreign code lengths."""
    codes = code_sets[name]
    hdr, host = _encode(mode, codes, False)
    hdr2, dev = _encode(mode, codes, True)
    assert hdr == hdr2 and np.array_equal(HR.codes_of_setup(enc_ref.SetupParams(hdr[2])), codes)
    want = _restated(mode, hdr)
    assert len(host) == len(dev) == len(want)
    for n, (a, b, w) in enumerate(zip(host, dev, want)):
        assert a["pkt"] == w, (mode, name, n, "host packer", len(a["pkt"]), len(w))
        assert b["pkt"] == w, (mode, name, n, "device packetiser", len(b["pkt"]), len(w))
        if w:
            assert a["pack"]["device"] == 0 and b["pack"]["device"] == 1
            assert np.array_equal(a["hist"]["count"], b["hist"]["count"]) and a["hist"]["huff"] == b["hist"]["huff"] == a["stats"]["huff"]
            assert (a["hist"]["device"], b["hist"]["device"]) == (0, 1)
            assert int(a["hist"]["count"].sum()) == a["stats"]["tokens_merged"]
    assert any(len(w) for w in want)


@pytest.mark.parametrize("pack", [False, True], ids=["host", "device"])
def test_histogram(hip, code_sets, pack):
    """A key and an inter packet: the histogram is tests/enc_huff_ref.py's over the restatement's tokens, huff[] is
    thip_enc_frame_stats.huff; a duplicate and a zero-byte packet give all zeros."""
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT, Encoder
    w, h, fmt, q = 64, 48, 0, 32
    frames = R.sequence("pan", w, h, fmt, 2, seed=4)
    e = Encoder(w, h, fmt, q, inter=True, device_pack=pack, huffman=code_sets["rotated"])
    setup = enc_ref.SetupParams(e.header_packets()[2])
    ref = R.InterEncoder(w, h, fmt, (0, 0, w, h), setup, 64, 6)
    zero = dict(count=np.zeros((5, 2, 32), np.int64), huff=[0] * 4, key=0, device=0)

    def same(a, b):
        return np.array_equal(a["count"], b["count"]) and all(a[k] == b[k] for k in ("huff", "key", "device"))
    try:
        for f, fr in enumerate(frames):
            if f == 0:
                assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, 1)[0] == 0
            e.encode(fr)
            pkt = e.packetout(False)[0]
            want = ref.frame(fr, q, dups=1 if f == 0 else 0)
            words = want["words"] if f else enc_ref.encode_frame(fr, w, h, fmt, (0, 0, w, h), q, setup)["words"]
            assert pkt == want["packet"] and len(pkt)
            got = e.token_hist()
            assert np.array_equal(got["count"], HR.hist_of_words(words)), f
            assert got["huff"] == e.stats()["huff"] == want["huff"] if f else got["huff"] == e.stats()["huff"]
            assert (got["key"], got["device"]) == (int(f == 0), int(pack))
            if f == 0:
                assert e.packetout(False)[0] == b"" and same(e.token_hist(), zero)   # the duplicate
        e.encode([np.ascontiguousarray(a) for a in e.recon()])   # the frame IS the reconstruction: nothing is coded
        assert e.packetout(True)[0] == b"" and same(e.token_hist(), zero)
    finally:
        ref.close()
        e.close()


def _deep_eob_codes():
    """The comb with token 6 (EOB runs of 32..4095, 12 extra bits) at a 31-bit code in every set: a 43-bit token."""
    codes = HR.comb_codes(lambda h: HR.comb_order(h, last=6))
    assert (codes[:, 6, 1] == 31).all()
    return codes


@pytest.mark.parametrize("pack", [False, True], ids=["host", "device"])
def test_the_43_bit_token_in_a_packet(hip, pack):
    """A flat 1024 x 64 key frame is one DC token and EOB runs of thousands: token 6 with its 12 extra bits under a 31-bit code.  The
    packet is the restatement's and decodes to a flat picture (the DC step at quality 63 is 16, an eighth of it a pixel: within 1)."""
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    w, h, fmt, q = 1024, 64, 0, 63
    frame = [np.full(s, v, np.uint8) for s, v in zip(enc_ref.plane_shapes(w, h, fmt), (90, 140, 60))]
    e = Encoder(w, h, fmt, q, device_pack=pack, huffman=_deep_eob_codes())
    hdr = e.header_packets()
    e.encode(frame)
    pkt = e.packetout(True)[0]
    hist, st = e.token_hist(), e.pack_stats()
    e.close()
    want = enc_ref.encode_frame(frame, w, h, fmt, (0, 0, w, h), q, enc_ref.SetupParams(hdr[2]))
    assert pkt == want["packet"]
    assert st["device"] == int(pack) and hist["count"][:, :, 6].sum() >= 1 and np.array_equal(hist["count"], HR.hist_of_words(want["words"]))
    dec = Decoder(hdr)
    assert dec.packetin(pkt)[0] == 0
    pic = dec.ycbcr_out()
    dec.close()
    for p, v in enumerate((90, 140, 60)):
        assert pic[p].min() == pic[p].max() and abs(int(pic[p][0, 0]) - v) <= 1, p


@pytest.mark.parametrize("groups,phase", [(1, 7), (2, 0)])
def test_the_43_bit_token_in_one_tile(hip, groups, phase):
    """thip_enc_pack_tokens on one tile of 256 tokens with seven runs of 32 EOBs, so seven 43-bit tokens -- the first of them with
    the AC table indices in front, 51 bits -- under the same codes: packref's bytes, and nothing written beyond the packet."""
    from tests.test_gpu_pack_direct import check
    codes = _deep_eob_codes()
    tables = (codes[..., 0].astype(np.uint32), codes[..., 1].astype(np.uint8))
    rng = np.random.default_rng(6)
    ll = P.lists_from({(0, 0): 20, (1, 0): 120, (1, 1): 60, (7, 2): 56})
    m = np.zeros(256, bool)
    for r in range(7):
        m[20 + r * 33:20 + r * 33 + 32] = True   # (the first run starts where index 1 does)
    words = P.stream(ll, m, rng)
    rec = check(hip, words, ll, tables, groups, phase)
    merged = P.merge(words, ll)
    assert sum(1 for t in merged if t[2] == 6) == 7 and rec["merged"] == 256 - 7 * 31


def _pass(w, h, fmt, q, frames, codes, pack=None, **kw):
    """-> headers, per frame (packet, reconstruction, token bits, histogram)."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, q, inter=True, device_pack=pack, huffman=codes, **kw)
    hdr, out = e.header_packets(), []
    for f, fr in enumerate(frames):
        e.encode(fr)
        pkt = e.packetout(f == len(frames) - 1)[0]
        out.append((pkt, e.recon(), e.pack_stats()["token_bits"], e.token_hist()))
    e.close()
    return hdr, out


@pytest.mark.parametrize("w,h,fmt,pack", [(64, 48, 0, False), (80, 64, 3, True)])
def test_two_passes_end_to_end(hip, w, h, fmt, pack):
    """Pass one with the built-in codes, train_huffman on its histograms, pass two in quality mode with no RD feature: the same
    reconstruction frame for frame, Sigma token_bits down by exactly bits_start - bits_end, and the pass-two stream decodes in the
    reference decoder to th_decode_*'s pictures."""
    from oracle import ref
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import train_huffman
    frames = R.sequence("pan", w, h, fmt, 5, seed=w)
    _, one = _pass(w, h, fmt, 40, frames, None, pack, all_modes=True)
    codes, st = train_huffman([x[3] for x in one])
    hdr, two = _pass(w, h, fmt, 40, frames, codes, pack, all_modes=True)
    assert st["bits_end"] < st["bits_start"]
    for f, (a, b) in enumerate(zip(one, two)):
        assert not refcmp.diff_planes(a[1], b[1]), f
        assert np.array_equal(a[3]["count"], b[3]["count"]), f
    assert sum(a[2] for a in one) - sum(b[2] for b in two) == st["bits_start"] - st["bits_end"]
    assert sum(len(b[0]) for b in two) < sum(len(a[0]) for a in one)
    dec, rd = Decoder(hdr), ref.RefDecoder(hdr) if ref.available() else None
    for f, b in enumerate(two):
        assert dec.packetin(b[0])[0] == 0, f
        pic = dec.ycbcr_out()
        assert not refcmp.diff_planes(pic, b[1]), f
        if rd:
            assert rd.packetin(b[0])[0] == 0, f
            assert not refcmp.diff_planes(pic, rd.ycbcr_out()), f
    dec.close()
    if rd:
        rd.close()


@pytest.mark.parametrize("name", ["comb", "trained"])
def test_reference_encoder_streams_under_these_codes_decode_here(hip, code_sets, name):
    """The other direction: the reference encoder, given the codes, makes a stream whose pictures in th_decode_* are the reference
    decoder's -- the front end has met trees 31 deep."""
    from oracle import ref
    from theora_amd import encoder as E
    from theora_amd.decoder import Decoder
    refcmp.need_ref()
    w, h, fmt = 80, 64, 0
    codes = code_sets[name]
    r = ref.RefEncoder(w, h, fmt, pic=ODD, quality=40, kf_interval=4)
    buf = E._huff_codes_in(codes)
    assert r._L.th_encode_ctl(r._enc, 0, C.byref(buf), C.sizeof(buf)) == 0
    hdr = r.header_packets()
    assert np.array_equal(HR.codes_of_setup(enc_ref.SetupParams(hdr[2])), codes)
    frames = refcmp.moving("natural", w, h, fmt, 5, seed=3)
    dec, rd = Decoder(hdr), ref.RefDecoder(hdr)
    for f, fr in enumerate(frames):
        for pkt, gp in r.encode(fr, last=f == len(frames) - 1):
            want = rd.packetin(pkt)
            assert want[0] >= 0 and dec.packetin(pkt) == want, f
            assert not refcmp.diff_planes(dec.ycbcr_out(), rd.ycbcr_out()), f
    r.close()
    dec.close()
    rd.close()


def test_encoder_example_train_huffman(hip, tmp_path):
    """examples/encoder_example_hip.c --train-huffman writes the stream of the Python encoder's two runs (the histograms with the
    built-in codes, train_huffman with 8 rounds, the input again); a pipe for input is refused."""
    import os
    import subprocess
    from tests.test_gpu_encoder import _compile, _y4m
    from theora_amd.decoder import ogg_packets
    from theora_amd.encoder import train_huffman
    w, h, fmt, q = 64, 48, 0, 32
    frames = R.sequence("pan", w, h, fmt, 4, seed=1)
    _, one = _pass(w, h, fmt, q, frames, None, keyframe_interval=3)
    codes, _ = train_huffman([x[3] for x in one], rounds=8)
    hdr, two = _pass(w, h, fmt, q, frames, codes, keyframe_interval=3)
    exe = _compile(tmp_path, "encoder_example_hip")
    (tmp_path / "in.y4m").write_bytes(_y4m(frames, w, h, "420jpeg"))
    args = [exe, "-q", str(q), "-k", "3", "--train-huffman", "-o", str(tmp_path / "out.ogv")]
    r = subprocess.run(args + [str(tmp_path / "in.y4m")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "trained on 4 packets" in r.stderr, r.stderr[-2000:]
    packets, (bad, gaps) = ogg_packets((tmp_path / "out.ogv").read_bytes())
    assert (bad, gaps) == (0, 0) and [p[1] for p in packets] == hdr + [x[0] for x in two]
    os.mkfifo(tmp_path / "pipe")
    fd = os.open(tmp_path / "pipe", os.O_RDWR)   # (keeps the example's open from waiting for a writer)
    try:
        r = subprocess.run(args + [str(tmp_path / "pipe")], capture_output=True, text=True, timeout=120)
    finally:
        os.close(fd)
    assert r.returncode == 1 and "seekable" in r.stderr
