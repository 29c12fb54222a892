"""th_encode_* on the GPU: the packets equal tests/enc_ref.py's restatement byte for byte, decode to the oracle's pictures, keep
their granule positions and duplicates straight, take device input in stream order, and do not depend on other threads."""
import threading

import numpy as np
import pytest

import oracle
from tests import enc_ref, streamgen
from tests.test_thirdparty_decoder import browser  # noqa: F401 -- the fixture (skips where that browser cannot run)


def _encode(w, h, fmt, quality, planes, pic=None, device_input=False, kfgshift=6, dups=None):
    """Headers, and per frame (packet, granulepos, stats) of encoding `planes` (a list of frames)."""
    from theora_amd.encoder import TH_ENCCTL_SET_DUP_COUNT, Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, kfgshift=kfgshift)
    hdr = e.header_packets()
    out = []
    for f, fr in enumerate(planes):
        if dups and dups[f]:
            assert e.ctl(TH_ENCCTL_SET_DUP_COUNT, dups[f])[0] == 0
        if device_input:
            import torch
            e.encode([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in fr])
        else:
            e.encode(fr)
        last = f == len(planes) - 1
        while True:
            r = e.packetout(last)
            if r is None:
                break
            out.append((r[0], r[1], e.stats(), r[3]))
    e.close()
    return hdr, out


CASES = [   # (w, h, fmt, pic, quality, content)
    (16, 16, 0, None, 32, "noise"),
    (176, 144, 0, None, 0, "natural"), (176, 144, 0, None, 16, "gradient"), (176, 144, 0, None, 48, "natural"),
    (176, 144, 2, None, 63, "natural"), (176, 144, 3, None, 32, "noise"), (176, 144, 3, None, 63, "flat"),
    (64, 48, 0, (1, 2, 61, 45), 32, "natural"), (64, 48, 2, (1, 2, 61, 45), 48, "noise"), (64, 48, 3, (1, 2, 61, 45), 16, "gradient"),
    (1280, 720, 0, None, 48, "natural"),
    (1920, 1088, 0, (0, 0, 1920, 1080), 16, "natural"),
    (176, 144, 2, None, 0, "flat"), (176, 144, 2, None, 63, "gradient"), (176, 144, 3, None, 0, "gradient"),
    (176, 144, 3, None, 16, "natural"), (176, 144, 0, None, 63, "noise"), (176, 144, 2, None, 32, "noise"),
    (1280, 720, 2, None, 0, "noise"), (1920, 1088, 3, (0, 0, 1920, 1080), 32, "natural"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality,kind", CASES)
def test_packets_equal_the_restatement(hip, w, h, fmt, pic, quality, kind):
    p = pic or (0, 0, w, h)
    frame = enc_ref.picture(kind, w, h, fmt, p, seed=w + quality)
    hdr, out = _encode(w, h, fmt, quality, [frame], pic=pic)
    setup = enc_ref.SetupParams(hdr[2])
    ref = enc_ref.encode_frame(frame, w, h, fmt, p, quality, setup)
    pkt, gp, st, eos = out[0]
    assert st["overflow"] == 0
    assert (st["tokens"], st["tokens_merged"], st["huff"]) == (ref["tokens"], ref["tokens_merged"], ref["huff"])
    assert pkt == ref["packet"]
    # the same frame as a picture-size buffer, and from device memory
    if pic is not None and w * h <= 176 * 144:
        small = [f[y0:y0 + ch, x0:x0 + cw] for f, (x0, y0, cw, ch) in
                 zip(frame, [enc_ref.chroma_region(p, fmt, q) for q in range(3)])]
        assert _encode(w, h, fmt, quality, [small], pic=pic)[1][0][0] == pkt
        assert _encode(w, h, fmt, quality, [small], pic=pic, device_input=True)[1][0][0] == pkt
    assert _encode(w, h, fmt, quality, [frame], pic=pic, device_input=True)[1][0][0] == pkt


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fmt,pic,quality", [(176, 144, 0, None, 20), (64, 48, 2, (1, 2, 61, 45), 40),
                                                  (96, 64, 3, (3, 1, 90, 60), 63)])
def test_packets_decode_to_the_oracles_picture(hip, w, h, fmt, pic, quality):
    from theora_amd import _lib
    from theora_amd.decoder import Decoder
    p = pic or (0, 0, w, h)
    frames = [enc_ref.picture(k, w, h, fmt, p, seed=s) for s, k in enumerate(("natural", "noise"))]
    hdr, out = _encode(w, h, fmt, quality, frames, pic=pic)
    setup = enc_ref.SetupParams(hdr[2])
    dec = Decoder(hdr)
    ost = oracle.State(w, h, fmt)
    refs = []
    for fr, (pkt, gp, st, eos) in zip(frames, out):
        ref = enc_ref.encode_frame(fr, w, h, fmt, p, quality, setup)
        refs.append(ref)
        assert dec.packetin(pkt)[0] == 0
        assert enc_ref.oracle_decode(ost, ref) == 0
        got = dec.ycbcr_out()
        for pli in range(3):
            assert np.array_equal(got[pli], ost.get_plane(oracle.FRAME_PREV, pli)[::-1]), pli
    dec.close()
    # slot-trace mode: the coefficients the host front end hands the backend are enc_ref's dequantised levels
    L = _lib.load()
    assert L.thip_set_option(b"fe_trace_backend", 1) == 0
    try:
        dec = Decoder(hdr)
        for ref, (pkt, gp, st, eos) in zip(refs, out):
            dec.packetin(pkt)
            t = dec.slot_trace()
            assert np.array_equal(t["fragi"], ref["coded_order"])
            want = np.zeros((len(ref["coded_order"]), 64), np.int64)
            want[:, enc_ref.ZIGZAG] = ref["levels"] * ref["dequant"][ref["plane_of"]]
            want[:, 0] = ref["levels"][:, 0]
            assert np.array_equal(t["coeffs"].astype(np.int64), want)
        dec.close()
    finally:
        L.thip_set_option(b"fe_trace_backend", 0)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


# measured on the MI355X, natural image 176x144: (quality-63 PSNR Y, Cb, Cr in dB, quality-48 bytes)
QUALITY_FLOOR = {0: ((47.79, 45.44, 44.69), 7338), 2: ((47.79, 45.97, 44.67), 9069), 3: ((47.79, 45.57, 44.67), 12894)}


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_bytes_and_psnr_grow_with_quality(hip, fmt):
    from theora_amd.decoder import Decoder
    w, h = 176, 144
    frame = enc_ref.picture("natural", w, h, fmt, seed=7)
    rows = []
    for q in (0, 8, 16, 24, 32, 40, 48, 56, 63):
        hdr, out = _encode(w, h, fmt, q, [frame])
        dec = Decoder(hdr)
        dec.packetin(out[0][0])
        got = dec.ycbcr_out()
        dec.close()
        rows.append((q, len(out[0][0])) + tuple(_psnr(got[p], frame[p]) for p in range(3)))
    print("fmt %d quality bytes psnr_y psnr_cb psnr_cr:" % fmt, [(r[0], r[1]) + tuple(round(x, 2) for x in r[2:]) for r in rows])
    for a, b in zip(rows, rows[1:]):
        assert b[1] >= a[1], (a, b)
        for p in range(3):
            assert b[2 + p] >= a[2 + p] - 1e-9, (a, b)
    psnr63, bytes48 = QUALITY_FLOOR[fmt]   # 1 dB below / 5 % above what was measured
    r63, r48 = rows[-1], rows[-3]
    assert all(r63[2 + p] >= psnr63[p] - 1.0 for p in range(3)), r63
    assert r48[1] <= bytes48 * 1.05, r48


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 6])
def test_granule_positions_and_duplicates(hip, shift):
    from theora_amd.decoder import Decoder
    w, h, fmt = 64, 48, 0
    frames = [enc_ref.picture(k, w, h, fmt, seed=s) for s, k in enumerate(("natural", "gradient", "noise"))]
    hdr, out = _encode(w, h, fmt, 63, frames, kfgshift=shift, dups=[2, 0, 1])
    assert [len(o[0]) == 0 for o in out] == [False, True, True, False, False, True]
    assert [o[3] for o in out] == [0, 0, 0, 0, 0, 1]
    assert all(o[2]["overflow"] == 0 for o in out)
    dec = Decoder(hdr)
    for pkt, gp, st, eos in out:
        rc, dgp = dec.packetin(pkt)
        assert rc == (1 if len(pkt) == 0 else 0)
        assert gp == dgp
    dec.close()


@pytest.mark.gpu
def test_no_overflow_on_noise_at_quality_63(hip):
    for fmt in (0, 3):
        frame = enc_ref.picture("noise", 128, 128, fmt, seed=3)
        _, out = _encode(128, 128, fmt, 63, [frame])
        assert out[0][2]["overflow"] == 0


@pytest.mark.gpu
def test_transcode_on_the_device(hip):
    """Decode a streamgen stream, write each picture with thip_picture_out into device tensors on a side stream, encode them from
    there: the packets equal those of the same pictures from the host."""
    import torch
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    w, h, fmt = 176, 144, 0
    st = streamgen.Stream(w, h, fmt, 11)
    dec = Decoder(st.header_packets())
    side = torch.cuda.Stream()
    e_dev, e_host = Encoder(w, h, fmt, 40), Encoder(w, h, fmt, 40)
    assert e_dev.header_packets() == e_host.header_packets()
    compared = 0
    for f in range(4):
        pkt, truth = st.frame(0 if f == 0 else 1, density=0.6)
        assert dec.packetin(pkt)[0] in (0, 1), f   # (TH_DUPFRAME: the picture is the previous one again)
        planes = dec.picture(fmt="ycbcr", crop=True, stream=side)
        e_dev.encode(planes, stream=side)
        e_host.encode(dec.ycbcr_out())
        a, b = e_dev.packetout(), e_host.packetout()
        assert a[0] == b[0] and a[1] == b[1], f
        compared += 1
    assert compared == 4
    for x in (dec, e_dev, e_host):
        x.close()


@pytest.mark.gpu
def test_encoders_on_two_threads(hip):
    w, h = 176, 144
    jobs = [(0, 30, [enc_ref.picture("natural", w, h, 0, seed=s) for s in range(4)]),
            (3, 50, [enc_ref.picture("noise", w, h, 3, seed=s) for s in range(4)])]
    alone = [_encode(w, h, fmt, q, frs)[1] for fmt, q, frs in jobs]
    got = [None, None]

    def run(i):
        fmt, q, frs = jobs[i]
        got[i] = _encode(w, h, fmt, q, frs)[1]
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for a, b in zip(alone, got):
        assert [(x[0], x[1]) for x in a] == [(x[0], x[1]) for x in b]


def _y4m(frames, w, h, tag):
    head = ("YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s\n" % (w, h, tag)).encode()
    return head + b"".join(b"FRAME\n" + b"".join(np.ascontiguousarray(p).tobytes() for p in fr) for fr in frames)


def _compile(tmp_path, name):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / name
    cc = subprocess.run(["gcc", "-O1", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", name + ".c"),
                         "-L" + os.path.join(root, "theora_amd"), "-ltheora_hip", "-Wl,-rpath," + os.path.join(root, "theora_amd"),
                         "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    return str(exe)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,tag,w,h", [(0, "420jpeg", 170, 138), (3, "444", 61, 45), (2, "422", 96, 64)])
def test_encoder_example_matches_the_python_encoder(hip, tmp_path, fmt, tag, w, h):
    """examples/encoder_example_hip.c: a .y4m of any size -> .ogv.  Its packets are the Python encoder's (picture-size buffers,
    the frame padded to multiples of 16), and examples/dump_video_hip.c decodes the file to what the Python decoder gives."""
    import subprocess
    from theora_amd.decoder import Decoder, ogg_packets
    from theora_amd.encoder import Encoder
    enc_exe, dump_exe = _compile(tmp_path, "encoder_example_hip"), _compile(tmp_path, "dump_video_hip")
    fw, fh = (w + 15) & ~15, (h + 15) & ~15
    pic = (0, 0, w, h)
    frames = [enc_ref.picture(k, fw, fh, fmt, pic, picture_size=True, seed=s)
              for s, k in enumerate(("natural", "noise", "gradient", "natural"))]
    (tmp_path / "in.y4m").write_bytes(_y4m(frames, w, h, tag))
    r = subprocess.run([enc_exe, "-q", "40", "-o", str(tmp_path / "out.ogv"), str(tmp_path / "in.y4m")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "4 frames" in r.stderr
    got, (bad, gaps) = ogg_packets((tmp_path / "out.ogv").read_bytes())
    assert (bad, gaps) == (0, 0)
    e = Encoder(fw, fh, fmt, 40, pic=pic)
    want = e.header_packets()
    gps = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        pkt = e.packetout(f == len(frames) - 1)
        want.append(pkt[0])
        gps.append(pkt[1])
    e.close()
    assert [g[1] for g in got] == want
    assert got[0][2] == 1 and got[-1][3] == 1 and got[-1][4] == gps[-1]
    # decode: dump_video's YUV4MPEG2 (the picture region) equals the Python decode of the same packets
    r = subprocess.run([dump_exe, "--crop", "-o", str(tmp_path / "out.y4m"), str(tmp_path / "out.ogv")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    data = (tmp_path / "out.y4m").read_bytes()
    head, _, rest = data.partition(b"\n")
    assert b" W%d H%d " % (w, h) in head
    dec = Decoder(want[:3])
    shapes = [(enc_ref.chroma_region(pic, fmt, q)[3], enc_ref.chroma_region(pic, fmt, q)[2]) for q in range(3)]
    fsz = 6 + sum(a * b for a, b in shapes)
    assert len(rest) == fsz * len(frames)
    for f, pkt in enumerate(want[3:]):
        assert dec.packetin(pkt)[0] == 0
        ours = dec.ycbcr_out()
        rec, off = rest[f * fsz:(f + 1) * fsz], 6
        assert rec[:6] == b"FRAME\n"
        for q, (ph, pw) in enumerate(shapes):
            plane = np.frombuffer(rec, np.uint8, ph * pw, off).reshape(ph, pw)
            off += ph * pw
            assert np.array_equal(plane, ours[q][:ph, :pw]), (f, q)
    dec.close()


@pytest.mark.gpu
def test_ffmpeg_in_chromium_plays_an_encoded_clip(hip, browser):
    """A decoder outside this project: FFmpeg's Theora decoder in the Chromium that kaleido bundles plays a 4:4:4 clip of the
    encoder's, and its frames equal the oracle's decode within RGB rounding (the comparison of tests/test_thirdparty_decoder.py;
    skips where that browser cannot run)."""
    from tests import test_thirdparty_decoder as tp
    from theora_amd.encoder import Encoder, ogg_stream
    w, h, fmt, n, q = 64, 48, 3, 6, 40
    frames = []
    for s in range(n):
        y = enc_ref.content("natural", (h, w), seed=20 + s)
        c = [np.clip(128 + (enc_ref.content("natural", (h, w), seed=40 + 2 * s + k).astype(np.int64) - 110) // 4, 0, 255)
             .astype(np.uint8) for k in range(2)]
        frames.append([y] + c)
    e = Encoder(w, h, fmt, q)
    hdr = e.header_packets()
    setup = enc_ref.SetupParams(hdr[2])
    data, want = [], []
    ost = oracle.State(w, h, fmt)
    for f, fr in enumerate(frames):
        e.encode(fr)
        pkt, gp, _, eos = e.packetout(f == n - 1)
        data.append((pkt, gp, eos))
        ref = enc_ref.encode_frame(fr, w, h, fmt, (0, 0, w, h), q, setup)
        assert ref["packet"] == pkt
        assert enc_ref.oracle_decode(ost, ref) == 0
        want.append([ost.get_plane(oracle.FRAME_PREV, p)[::-1].astype(np.float64) for p in range(3)])
    e.close()
    out = tp.play(browser, ogg_stream(hdr, data), n)
    assert (out["w"], out["h"]) == (w, h) and len(out["frames"]) == n
    exact = 0
    for f in range(n):
        scores = tp.compare({"frames": [out["frames"][f]] * n}, want, w, h)
        g = min(range(n), key=lambda i: scores[i][0])
        mean, worst_block, share = scores[g]
        assert abs(g - f) <= 1, (f, g)
        assert share > 0.15, (f, share)
        assert mean < 0.6 and worst_block < 1.5, (f, g, mean, worst_block)
        exact += g == f
    assert exact >= n - 2
