"""th_encode_* two-pass on the GPU (include/theoraenc_hip.h, "Two-pass"): the first pass changes no packet and records the curves
tests/enc_2pass_ref.py restates; the second pass's choices and packets equal the restatement's, follow the recorded frame types,
land on the file's budget closer than one pass does, and spend it more evenly; misuse on a live context is refused cleanly."""
import numpy as np
import pytest

from tests import enc_2pass_ref as TP
from tests import enc_inter_ref as R
from tests import enc_ref
from tests.test_gpu_encoder import _psnr

EINVAL = "returned -10"


def _dup(e, n):
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT
    assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, n)[0] == 0


def _first(w, h, fmt, frames, record=True, dups=None, quality=32, **kw):
    """One pass, with TH_ENCCTL_THIP_2PASS_OUT when `record`: headers, [(packet, granulepos)], the pass file, and per packet
    (two-pass stats, rate stats or None)."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, quality, **kw)
    hdr = e.header_packets()
    place = e.two_pass_out() if record else b""
    out, recs, stats, final = [], [], [], b""
    for f, fr in enumerate(frames):
        if dups and dups.get(f):
            _dup(e, dups[f])
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append((r[0], r[1]))
            stats.append((e.two_pass_stats(), e.rate_stats() if kw.get("bitrate") else None))
            if record:
                recs.append(e.two_pass_out())
                assert len(recs[-1]) == TP.RECORD_BYTES
                if not r[3]:
                    assert e.two_pass_out() == b""          # one record a packet
    if record:
        final = e.two_pass_out()                             # after the last packet's record: the finished header
        assert len(final) == len(place) == TP.HEADER_BYTES and e.two_pass_out() == b""
        assert TP.unpack_header(place)["fields"] == TP.unpack_header(final)["fields"]
    e.close()
    return hdr, out, final + b"".join(recs), stats


def _second(w, h, fmt, frames, passfile, bitrate, dups=None, chunk=None, recon=False, **kw):
    """The second pass: headers and per packet (packet, granulepos, rate stats, two-pass stats[, reconstruction])."""
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, 32, bitrate=bitrate, **kw)
    hdr = e.header_packets()
    fed = 0
    if chunk is None:
        fed = e.two_pass_in(passfile)
        assert fed == len(passfile)
    out = []
    for f, fr in enumerate(frames):
        while chunk is not None and e.two_pass_in(None) > 0:   # libtheora's loop: feed until the next frame can be taken
            assert fed < len(passfile)
            fed += e.two_pass_in(passfile[fed:fed + chunk])
        if dups and dups.get(f):
            _dup(e, dups[f])
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            out.append((r[0], r[1], e.rate_stats(), e.two_pass_stats()) + ((e.recon(),) if recon else ()))
    e.close()
    return hdr, out


# ---- pass 1 -----------------------------------------------------------------------------------------------------------------------
EVERYTHING = dict(inter=True, keyframe_interval=64, all_modes=True, auto_keyframes=True, device_pack=True, rd_modes=True, block_qi=6)
PASS1 = [   # (name, w, h, fmt, content, frames, Encoder arguments, dups)
    ("quality-key", 64, 48, 3, "pan", 4, dict(), None),
    ("quality-inter", 176, 144, 0, "pan", 6, dict(inter=True, keyframe_interval=4), None),
    ("bitrate-key", 64, 48, 3, "pan", 4, dict(bitrate=60000), None),
    ("bitrate-inter", 176, 144, 0, "cut", 10, dict(inter=True, keyframe_interval=4, bitrate=150000), None),
    ("quality-everything", 176, 144, 0, "cut", 10, dict(EVERYTHING), {3: 1}),
    ("bitrate-everything", 176, 144, 0, "cut", 10, dict(EVERYTHING, bitrate=400000), {3: 1}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,fmt,kind,n,kw,dups", PASS1, ids=[c[0] for c in PASS1])
def test_pass_one_changes_no_packet(hip, name, w, h, fmt, kind, n, kw, dups):
    """The packets and granule positions with TH_ENCCTL_THIP_2PASS_OUT on are those of the same run without it; the header's counts
    and sums are the records'; in bitrate mode the recorded curve is thip_enc_rate_stats.probe."""
    frames = R.sequence(kind, w, h, fmt, n, seed=5)
    _, plain, _, _ = _first(w, h, fmt, frames, record=False, dups=dups, **kw)
    _, got, data, stats = _first(w, h, fmt, frames, record=True, dups=dups, **kw)
    assert got == plain
    hdr, recs = TP.parse(data)
    assert data[:TP.HEADER_BYTES] == TP.finish_header(hdr["fields"], recs)
    assert hdr["fields"] == TP.fields_of(w, h, (0, 0, w, h), fmt, (30, 1), 6, kw.get("inter", False))
    assert hdr["dups"] == sum((dups or {}).values()) and hdr["frames"] == n
    keys = [k for k, r in enumerate(recs) if r["type"] == TP.KEY]
    for k, (r, (tp, rate), (pkt, gp)) in enumerate(zip(recs, stats, got)):
        assert tp["pass"] == 1 and tp["frame"] == k and tp["type"] == r["type"] and tp["recorded"] == r["E"]
        assert r["bits"] == 8 * len(pkt)
        if r["type"] == TP.DUP:
            assert r["E"] == [0] * 64 and not pkt
            continue
        assert tp["fresh"] == r["E"] and min(r["E"]) > 0 and r["E"][63] >= r["E"][0]
        if rate is not None:
            assert rate["probe"] == r["E"] and r["qi"] == rate["qi"]
            assert r["type"] == (TP.DROPPED if rate["dropped"] else TP.KEY if rate["key"] else TP.INTER)
        else:
            assert r["qi"] == 32 and r["type"] == (TP.INTER if pkt and pkt[0] & 0x40 else TP.KEY)
    if kw.get("auto_keyframes"):
        assert any(k > 0 for k in keys)       # the cut's key frame is in the records with the type it really had
    print(name, "types", [r["type"] for r in recs], "wait ms", ["%.3f" % s[0]["wait_ms"] for s in stats])


RECORDED = [   # (name, w, h, fmt, pic, frames, quality, bitrate, inter, kf, dups)
    ("quality-key-444", 64, 48, 3, (1, 2, 61, 45), 3, 40, None, False, None, None),
    ("quality-inter", 176, 144, 0, None, 6, 24, None, True, 4, {2: 1}),
    ("bitrate-inter", 176, 144, 0, None, 6, 32, 200000, True, 4, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,fmt,pic,n,quality,bitrate,inter,kf,dups", RECORDED, ids=[c[0] for c in RECORDED])
def test_recorded_curves_equal_the_restatement(hip, name, w, h, fmt, pic, n, quality, bitrate, inter, kf, dups):
    """The whole pass file -- every record's type, qi, bits and E[0..63] (enc_rate_ref.Probe on the restatement's reference), and
    the finished header -- equals the restatement's, byte for byte; so do the packets."""
    frames = R.sequence("pan", w, h, fmt, n, seed=9)
    if pic:
        reg = [enc_ref.chroma_region(pic, fmt, p) for p in range(3)]
        frames = [[np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in zip(fr, reg)] for fr in frames]
    kw = dict(pic=pic, inter=inter, keyframe_interval=kf if inter else None, bitrate=bitrate)
    hdr, got, data, _ = _first(w, h, fmt, frames, dups=dups, quality=quality, **kw)
    p1 = TP.Pass1(w, h, fmt, pic or (0, 0, w, h), enc_ref.SetupParams(hdr[2]), quality=None if bitrate else quality,
                  bitrate=bitrate, inter=inter, kf_interval=kf or 64)
    try:
        want = [x for f, fr in enumerate(frames) for x in p1.frame(fr, (dups or {}).get(f, 0))]
        assert [g[0] for g in got] == [x[0] for x in want]
        _, grecs = TP.parse(data)
        for k, (g, x) in enumerate(zip(grecs, want)):
            assert g == TP.unpack_record(x[1]), k
        assert data == p1.file()
    finally:
        p1.close()


# ---- pass 2 -----------------------------------------------------------------------------------------------------------------------
SECOND = [   # (name, w, h, fmt, frames, inter, kf, pass-1 quality, bitrate, dups, chunk)
    ("key-444", 64, 48, 3, 5, False, None, 32, 90000, None, 7),
    ("inter", 176, 144, 0, 8, True, 4, 40, 120000, {2: 1}, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,fmt,n,inter,kf,quality,bitrate,dups,chunk", SECOND, ids=[c[0] for c in SECOND])
def test_pass_two_equals_the_restatement(hip, name, w, h, fmt, n, inter, kf, quality, bitrate, dups, chunk):
    """Every qi, every correction, the budget left and every packet of the second pass equal the restatement's, with the pass file
    fed whole or in chunks of 7 bytes as TH_ENCCTL_THIP_2PASS_IN(NULL) asks for it."""
    frames = R.sequence("pan", w, h, fmt, n, seed=13)
    kw = dict(inter=inter, keyframe_interval=kf if inter else None)
    _, _, data, _ = _first(w, h, fmt, frames, dups=dups, quality=quality, **kw)
    hdr, got = _second(w, h, fmt, frames, data, bitrate, dups=dups, chunk=chunk, **kw)
    p2 = TP.Pass2(w, h, fmt, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), bitrate, data, inter=inter)
    try:
        want = [x for f, fr in enumerate(frames) for x in p2.frame(fr, (dups or {}).get(f, 0))]
    finally:
        p2.close()
    assert len(got) == len(want)
    for k, ((pkt, gp, rate, tp), (wpkt, st)) in enumerate(zip(got, want)):
        assert tp["pass"] == 2 and tp["frame"] == k
        if st.get("duplicate"):
            assert not pkt and rate["duplicate"] == 1 and tp["type"] == TP.DUP
            continue
        assert (rate["qi"], rate["key"], rate["probe"], rate["actual"], rate["corr"]) == \
            (st["qi"], st["key"], st["probe"], st["actual"], st["corr"]), k
        assert (tp["qi"], tp["fresh"], tp["recorded"], tp["corr"], tp["budget_left"], tp["recorded_left"]) == \
            (st["qi"], st["probe"], st["recorded"], st["corr"] + st["ratio"], st["budget_left"], st["recorded_left"]), k
        assert rate["dropped"] == 0 and rate["fullness_after"] == st["budget_left"]
        assert pkt == wpkt, k
    print(name, "qi", [g[2]["qi"] for g in got])


@pytest.mark.gpu
def test_pass_two_reconstruction_is_the_reference_decoders_picture(hip):
    from oracle import ref
    from tests import refcmp
    refcmp.need_ref()
    w, h, fmt, n = 176, 144, 0, 8
    frames = R.sequence("pan", w, h, fmt, n, seed=13)
    kw = dict(inter=True, keyframe_interval=4, all_modes=True, block_qi=4)
    _, _, data, _ = _first(w, h, fmt, frames, **kw)
    hdr, got = _second(w, h, fmt, frames, data, 150000, recon=True, **kw)
    rd = ref.RefDecoder(hdr)
    try:
        for f, (pkt, gp, rate, tp, recon) in enumerate(got):
            rc, rgp = rd.packetin(pkt)
            assert rc == (0 if pkt else 1) and rgp == gp, f
            bad = refcmp.diff_planes(recon, rd.ycbcr_out())
            assert not bad, (f, bad)
            refcmp.TALLY["frames"] += 1
    finally:
        rd.close()


@pytest.mark.gpu
def test_types_are_followed(hip):
    """A first pass whose cut detector placed key frames mid-clip: the second pass, at a target that moves qi by more than 10 from
    the first pass's 48, has its key frames at exactly the same indices (it measures nothing: cut_stats.measured is 0)."""
    from theora_amd.encoder import Encoder
    w, h, fmt, n = 64, 48, 0, 10
    frames = R.sequence("cut", w, h, fmt, n, seed=4)
    kw = dict(inter=True, keyframe_interval=64, auto_keyframes=True)
    _, first, data, _ = _first(w, h, fmt, frames, quality=48, **kw)
    _, recs = TP.parse(data)
    keys = [k for k, r in enumerate(recs) if r["type"] == TP.KEY]
    assert keys[0] == 0 and len(keys) > 1 and len(keys) < n
    bitrate = sum(8 * len(p) for p, _ in first) * 30 // n // 5
    e = Encoder(w, h, fmt, 32, bitrate=bitrate, **kw)
    e.header_packets()
    assert e.two_pass_in(data) == len(data)
    got, qis = [], []
    for f, fr in enumerate(frames):
        e.encode(fr)
        pkt = e.packetout(f == n - 1)[0]
        assert e.cut_stats()["measured"] == 0
        if e.rate_stats()["key"]:
            got.append(f)
            assert pkt and not pkt[0] & 0x40
        qis.append(e.rate_stats()["qi"])
    e.close()
    assert got == keys
    assert all(abs(q - 48) > 10 for q in qis), qis


def _one_pass(w, h, frames, bitrate, kf):
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, 0, 32, inter=True, keyframe_interval=kf, bitrate=bitrate, rate_buffer=12)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        pkt = e.packetout(f == len(frames) - 1)[0]
        out.append((pkt, e.rate_stats()))
    e.close()
    return hdr, out


def _y_psnr(hdr, packets, frames):
    from theora_amd.decoder import Decoder
    dec = Decoder(hdr)
    ps = []
    for pkt, fr in zip(packets, frames):
        dec.packetin(pkt)
        ps.append(_psnr(dec.ycbcr_out()[0], fr[0]))
    dec.close()
    return ps


# |8 sum bytes - B| of the restated two-pass encoder on the CPU, per target as a fraction of the way from the
# clip's quality-8 rate to its quality-56 rate
MEASURED_DEVIATION = {4: 1208, 2: 2192}


@pytest.fixture(scope="module")
def uneven(hip):
    """The 24-frame uneven clip, its first pass at quality 32 (K = 12) and its quality-8 and quality-56 rates."""
    frames = TP.uneven_clip(24)
    kw = dict(inter=True, keyframe_interval=12)
    rates = []
    for q in (8, 56):
        _, out, _, _ = _first(176, 144, 0, frames, record=False, quality=q, **kw)
        rates.append(sum(len(p) for p, _ in out) * 8 * 30 // 24)
    _, _, data, _ = _first(176, 144, 0, frames, quality=32, **kw)
    return frames, data, rates[0], rates[1]


@pytest.mark.gpu
@pytest.mark.parametrize("part", [4, 2])
def test_the_total_lands_and_the_spend_is_even(uneven, part):
    """Two targets between the clip's quality-8 and quality-56 rates, a quarter and half of the way up: |8 sum bytes - B| is within
    twice what the restatement measured on the CPU (1208 and 2192 bits), within the one-pass bound R / 2 + T (R = 12 T), and
    smaller than the one-pass stream's deviation from N T on the same clip and target (2088 and 10680 bits there); the minimum and
    the mean Y PSNR are higher than the one-pass stream's (the restatement: by 1.88 and 0.77 dB at the lower target, by 1.19 and
    0.44 dB at the upper one).
    The spread of qi over the inter frames, max - min, is asserted smaller than the one-pass stream's at the lower target (2
    against 18), where the budget binds in the hard half that one pass cannot see coming.  At the upper target it is NOT smaller
    (12 against 10) and is printed only: the hard half's noise field moves by whole pixels, so a frame pays for a step of qi
    once and its successors get it free, which no per-frame curve recorded against another reference says; both controllers climb
    through that half as the bits they expected to need come back."""
    frames, data, lo, hi = uneven
    n = len(frames)
    bitrate = lo + (hi - lo) // part
    kw = dict(inter=True, keyframe_interval=12)
    hdr, got = _second(176, 144, 0, frames, data, bitrate, **kw)
    T = got[0][2]["target"]
    B = n * T
    dev = abs(sum(8 * len(g[0]) for g in got) - B)
    hdr1, one = _one_pass(176, 144, frames, bitrate, 12)
    dev1 = abs(sum(8 * len(p) for p, _ in one) - B)
    q2 = [g[2]["qi"] for g in got if not g[2]["key"]]
    q1 = [st["qi"] for _, st in one if not st["key"] and not st["dropped"]]
    ps2 = _y_psnr(hdr, [g[0] for g in got], frames)
    ps1 = _y_psnr(hdr1, [p for p, _ in one], frames)
    print("target %d bit/s (T %d, B %d): two-pass deviation %d, one-pass %d, bound %d; inter qi spread %d / %d; Y PSNR min %.3f mean "
          "%.3f / min %.3f mean %.3f" % (bitrate, T, B, dev, dev1, 6 * T + T, max(q2) - min(q2), max(q1) - min(q1), min(ps2),
                                         float(np.mean(ps2)), min(ps1), float(np.mean(ps1))))
    assert [g[2]["key"] for g in got] == [int(f % 12 == 0) for f in range(n)]
    assert dev <= 2 * MEASURED_DEVIATION[part]
    assert dev <= 6 * T + T
    assert dev < dev1
    assert min(ps2) > min(ps1) and np.mean(ps2) > np.mean(ps1)
    if part == 4:
        assert max(q2) - min(q2) < max(q1) - min(q1)


# ---- misuse -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misuse_on_a_live_context(hip):
    from theora_amd._lib import TheoraHipError
    from theora_amd.encoder import Encoder
    w, h, fmt = 64, 48, 0
    frames = R.sequence("pan", w, h, fmt, 4, seed=2)
    _, _, data, _ = _first(w, h, fmt, frames[:3])
    # records for fewer frames than are submitted: the fourth frame is refused, the context goes on answering and closes
    e = Encoder(w, h, fmt, 32, bitrate=80000)
    e.header_packets()
    assert e.two_pass_in(data) == len(data)
    for fr in frames[:3]:
        e.encode(fr)
        assert e.packetout(False)[0]
    with pytest.raises(TheoraHipError, match=EINVAL):
        e.encode(frames[3])
    assert e.packetout(True) is None and e.two_pass_stats()["frame"] == 2 and e.two_pass_in(None) == 0
    e.close()
    # a record short: the frame waits for it, and is taken once it is whole
    e = Encoder(w, h, fmt, 32, bitrate=80000)
    e.header_packets()
    assert e.two_pass_in(data[:-1]) == len(data) - 1
    for fr in frames[:2]:
        e.encode(fr)
        assert e.packetout(False)[0]
    assert e.two_pass_in(None) == 1
    with pytest.raises(TheoraHipError, match=EINVAL):
        e.encode(frames[2])
    assert e.two_pass_in(data[-1:]) == 1
    e.encode(frames[2])
    assert e.packetout(True)[3] == 1
    e.close()
    # either request after the first frame, and both on one context
    e = Encoder(w, h, fmt, 32, bitrate=80000)
    e.header_packets()
    e.encode(frames[0])
    for call in (lambda: e.two_pass_in(data), lambda: e.two_pass_in(None), e.two_pass_out):
        with pytest.raises(TheoraHipError, match=EINVAL):
            call()
    assert e.packetout(False)[0]
    for call in (lambda: e.two_pass_in(data), e.two_pass_out):
        with pytest.raises(TheoraHipError, match=EINVAL):
            call()
    assert e.two_pass_stats()["pass"] == 0
    e.encode(frames[1])
    assert e.packetout(True)[3] == 1
    e.close()
    e = Encoder(w, h, fmt, 32)
    e.header_packets()
    assert len(e.two_pass_out()) == TP.HEADER_BYTES
    e.encode(frames[0])
    with pytest.raises(TheoraHipError, match=EINVAL):
        e.two_pass_in(data)
    assert e.packetout(False)[0] and len(e.two_pass_out()) == TP.RECORD_BYTES
    with pytest.raises(TheoraHipError, match=EINVAL):
        e.two_pass_in(None)
    e.close()


# ---- the C example ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_encoder_example_two_pass_matches_the_python_encoder(hip, tmp_path):
    """examples/encoder_example_hip.c: --two-pass, and --first-pass then --second-pass, write the stream the Python encoder makes
    from the same two passes; the pass file --first-pass writes is the Python first pass's."""
    import subprocess
    from tests.test_gpu_encoder import _compile, _y4m
    from theora_amd.decoder import ogg_packets
    w, h, fmt, n = 96, 64, 0, 10
    frames = R.sequence("pan", w, h, fmt, n, seed=4)
    exe = _compile(tmp_path, "encoder_example_hip")
    y4m, pf, ogv = str(tmp_path / "in.y4m"), str(tmp_path / "pass.bin"), str(tmp_path / "out.ogv")
    (tmp_path / "in.y4m").write_bytes(_y4m(frames, w, h, "420jpeg"))
    kw = dict(inter=True, keyframe_interval=6)
    _, _, data, _ = _first(w, h, fmt, frames, quality=32, **kw)
    hdr, got = _second(w, h, fmt, frames, data, 40000, **kw)
    want = hdr + [g[0] for g in got]
    common = [exe, "-q", "32", "-k", "6"]
    for steps in ([["-V", "40", "--two-pass", "-o", ogv]],
                  [["--first-pass", pf], ["-V", "40", "--second-pass", pf, "-o", ogv]]):
        for args in steps:
            r = subprocess.run(common + args + [y4m], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
        packets, (bad, gaps) = ogg_packets((tmp_path / "out.ogv").read_bytes())
        assert (bad, gaps) == (0, 0)
        assert [p[1] for p in packets] == want
    assert (tmp_path / "pass.bin").read_bytes() == data
    r = subprocess.run(common + ["--second-pass", pf, y4m], capture_output=True, text=True, timeout=300)   # no -V: usage
    assert r.returncode == 1
