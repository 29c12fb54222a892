"""Frame side data (thip_frame_info_out) without a GPU: the numpy restatement (tests/frame_info_ref.py) pinned against values
worked out by hand, against what the encoder restatements chose for every macro block of the streams they make, against the
generator's ground truth, on the reference-made stream and on planted motion; the kernel's body run on the host under sanitizers;
and the argument checks that return before any state is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import enc_modes_ref as M
from tests import enc_ref, frame_info_ref as fr, refcmp, streamgen


@pytest.fixture()
def trace_env():
    """Contexts allocated inside the test record the slot calls instead of running them (option fe_trace_backend): no device."""
    from theora_amd import _lib
    L = _lib.load()
    old = L.thip_option(b"fe_trace_backend")
    assert L.thip_set_option(b"fe_trace_backend", 1) == 0
    yield
    L.thip_set_option(b"fe_trace_backend", old)


def test_restatement_by_hand():
    """One macro block of 4:2:0 (2 x 2 luma fragments, one of each chroma): fragment 0 is the BOTTOM left one."""
    f = fr.empty(16, 16, 0)
    # bottom left: from PREV, vector (+3, +5); bottom right: uncoded with stale bits; top left: intra with stale bits; top right: GOLD
    f["coded"][:] = [1, 0, 1, 1, 1, 1]
    f["refi"][:] = [fr.FRAME_PREV, fr.FRAME_GOLD, fr.FRAME_SELF, fr.FRAME_GOLD, fr.FRAME_PREV, fr.FRAME_SELF]
    f["mvx"][:] = [3, 9, -7, -31, -2, 1]
    f["mvy"][:] = [5, 9, 7, 31, 6, 1]
    f["last_zzi"][:] = [64, 17, 0, 1, 2, 3]
    got = fr.frame_info(f, 16, 16, 0, refs=fr.REF_PREV)
    assert got["kind"][0].tolist() == [[1, 3], [2, 0]] and got["kind"][1].tolist() == [[2]] and got["kind"][2].tolist() == [[1]]
    assert got["mv"][0].tolist() == [[[0, 0], [-31, -31]], [[3, -5], [0, 0]]]          # (vx, vy) = (mvx, -mvy)
    assert got["mv"][1].tolist() == [[[-2, -6]]] and got["mv"][2].tolist() == [[[0, 0]]]
    assert got["ncoef"][0].tolist() == [[0, 1], [64, 0]] and got["ncoef"][1].tolist() == [[2]]
    assert got["flow"].dtype == np.float16 and got["flow"].shape == (2, 16, 16) and got["valid"].shape == (16, 16)
    assert (got["valid"][:8, :8] == 1).all() and (got["valid"][:8, 8:] == 3).all() and (got["valid"][8:, :8] == 2).all()
    assert (got["valid"][8:, 8:] == 0).all()
    assert (got["flow"][0, 8:, :8] == 1.5).all() and (got["flow"][1, 8:, :8] == -2.5).all()
    assert (got["flow"][:, :8] == 0).all() and (got["flow"][:, 8:, 8:] == 0).all()     # GOLD not asked for, intra, uncoded
    both = fr.frame_info(f, 16, 16, 0, refs=fr.REF_PREV | fr.REF_GOLD, dtype=np.float32)
    assert both["flow"].dtype == np.float32 and (both["flow"][:, :8, 8:] == -15.5).all()
    none = fr.frame_info(f, 16, 16, 0, refs=0)
    assert not none["flow"].any() and np.array_equal(none["valid"], got["valid"])
    # a rectangle: pixels 7..8 of rows 6..9 touch all four luma fragments and the one chroma fragment
    r = fr.frame_info(f, 16, 16, 0, rect=(7, 6, 2, 4), refs=3)
    assert r["kind"][0].tolist() == [[1, 3], [2, 0]] and r["kind"][1].shape == (1, 1)
    assert r["valid"].tolist() == [[1, 3], [1, 3], [2, 0], [2, 0]]
    assert r["flow"][0].tolist() == [[0, -15.5], [0, -15.5], [1.5, 0], [1.5, 0]]
    r = fr.frame_info(f, 16, 16, 0, rect=(9, 0, 7, 8))
    assert r["kind"][0].tolist() == [[3]] and r["mv"][0].shape == (1, 1, 2) and r["flow"].shape == (2, 8, 7)


def test_shapes_follow_the_rule():
    import theora_amd
    for pf in (0, 2, 3):
        hd, vd = fr.decs(pf)
        for rect in ((0, 0, 48, 80), (1, 3, 45, 75), (7, 7, 2, 2), (15, 16, 1, 1), (8, 8, 8, 8), (9, 0, 37, 1)):
            x, y, w, h = rect
            s = theora_amd.frame_info_shapes(w, h, x, y, pf)
            assert s["flow"] == (2, h, w) and s["valid"] == (h, w)
            for p in range(3):
                c0, r0, fw, fh = fr.frag_rect(rect, p, pf)
                assert s["kind"][p] == (fh, fw) == s["ncoef"][p] and s["mv"][p] == (fh, fw, 2)
                # every fragment the rectangle's pixels fall into, and no other
                cols = sorted({(i >> (hd if p else 0)) >> 3 for i in range(x, x + w)})
                rows = sorted({(j >> (vd if p else 0)) >> 3 for j in range(y, y + h)})
                assert cols == list(range(c0, c0 + fw)) and rows == list(range(r0, r0 + fh))


def _word0(f):
    """The frag_info word0 of every fragment (include/theora_hip.h) from the per-fragment arrays, with stale bits where allowed."""
    w = (f["coded"].astype(np.uint32) | (f["refi"].astype(np.uint32) & 3) << 1 | (f["last_zzi"].astype(np.uint32) & 127) << 8
         | (f["mvx"].astype(np.int64) & 0xFF).astype(np.uint32) << 16 | (f["mvy"].astype(np.int64) & 0xFF).astype(np.uint32) << 24)
    return w | np.where(f["last_zzi"] < 2, np.uint32(8), np.uint32(0))


def test_words_and_arrays_agree():
    rng = np.random.default_rng(3)
    f = fr.empty(48, 80, 2)
    n = f["coded"].size
    f["coded"][:] = rng.random(n) < 0.7
    f["refi"][:] = rng.integers(0, 3, n)
    f["mvx"][:], f["mvy"][:] = rng.integers(-31, 32, n), rng.integers(-31, 32, n)
    f["last_zzi"][:] = rng.integers(0, 65, n)
    g = fr.from_word0(_word0(f))
    for rect in (None, (1, 3, 45, 75)):
        a, b = fr.frame_info(f, 48, 80, 2, rect, 3), fr.frame_info(g, 48, 80, 2, rect, 3)
        for key in ("kind", "mv", "ncoef"):
            assert all(np.array_equal(x, y) for x, y in zip(a[key], b[key]))
        assert np.array_equal(a["flow"], b["flow"]) and np.array_equal(a["valid"], b["valid"])


@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_generated_streams_against_their_ground_truth(trace_env, fmt):
    """streamgen's packets through a slot-trace context: the per-fragment arrays from the trace are the generator's own."""
    from theora_amd.decoder import Decoder
    w, h = 48, 80
    st = streamgen.Stream(w, h, fmt, seed=11 + fmt)
    dec = Decoder(st.header_packets())
    checked = 0
    for k in range(6):
        pkt, truth = st.frame(0 if k == 0 else 1, density=[0.9, 0.5, 0.15][k % 3])
        rc, _ = dec.packetin(pkt)
        if truth["dup"]:
            continue
        assert rc == 0
        f = fr.from_trace(dec.slot_trace(), w, h, fmt)
        coded = truth["coded"].astype(bool)
        assert np.array_equal(f["coded"], coded)
        assert np.array_equal(f["refi"][coded], truth["refi"][coded])
        inter = coded & (truth["refi"] != fr.FRAME_SELF)
        assert np.array_equal(f["mvx"][inter], truth["mvx"][inter]) and np.array_equal(f["mvy"][inter], truth["mvy"][inter])
        got = fr.frame_info(f, w, h, fmt, (1, 3, 45, 75), 3)
        # the dense outputs are the luma maps, every fragment eight pixels square
        full = fr.frame_info(f, w, h, fmt, None, 3, np.float32)
        assert np.array_equal(full["valid"], np.kron(full["kind"][0], np.ones((8, 8), np.uint8)))
        assert np.array_equal(full["flow"][0], np.kron(full["mv"][0][..., 0].astype(np.float32) / 2, np.ones((8, 8), np.float32)))
        assert np.array_equal(full["flow"][1], np.kron(full["mv"][0][..., 1].astype(np.float32) / 2, np.ones((8, 8), np.float32)))
        assert np.array_equal(got["valid"], full["valid"][3:78, 1:46]) and np.array_equal(got["flow"], full["flow"][:, 3:78, 1:46].astype(np.float16))
        checked += 1
    assert checked >= 4
    dec.close()


@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_eight_mode_streams_against_the_words_the_encoder_chose(trace_env, fmt):
    """The eight-mode encoder restatement's stream (48 x 80, the picture at an odd offset) through a slot-trace context: kind,
    vectors -- the chroma vectors of spec 7.5.2 for INTER_MV_FOUR among them -- and the coded set follow from the macro-block modes
    and vectors the restatement itself chose."""
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    w, h, pic, q = 48, 80, (1, 3, 45, 75), 40
    e = Encoder(w, h, fmt, q, pic=pic)
    hdr = e.header_packets()
    e.close()
    setup = enc_ref.SetupParams(hdr[2])
    reg = [enc_ref.chroma_region(pic, fmt, p) for p in range(3)]
    seen = np.zeros(8, np.int64)
    for kind_of_clip in ("shear", "uncover", "pan"):
        frames = M.sequence(kind_of_clip, w, h, fmt, 5, seed=2)
        frames = [[np.ascontiguousarray(a[y0:y0 + ch, x0:x0 + cw]) for a, (x0, y0, cw, ch) in zip(f, reg)] for f in frames]
        enc = M.ModesEncoder(w, h, fmt, pic, setup, 64, 6)
        dec = Decoder(hdr)
        geo = enc.geo
        try:
            for k, planes in enumerate(frames):
                r = enc.frame(planes, q)
                rc, _ = dec.packetin(r["packet"])
                assert rc == (0 if r["packet"] else 1)
                if not r["packet"]:
                    continue
                f = fr.from_trace(dec.slot_trace(), w, h, fmt)
                got = fr.frame_info(f, w, h, fmt, None, 3)
                if r["key"]:
                    assert all((kd == 1).all() for kd in got["kind"]) and not got["flow"].any() and (got["valid"] == 1).all()
                    assert not any(m.any() for m in got["mv"])
                    continue
                pix, ms = r["pix"], r["search"]
                seen += np.bincount(pix, minlength=8)
                coded = np.zeros(geo.nfrags, bool)
                coded[r["coded_fragis"]] = True
                fpix = pix[geo.mb_of]
                kind = np.where(~coded, 0, np.where(fpix == M.INTRA, 1, np.where((fpix == M.GOLDEN_NOMV) | (fpix == M.GOLDEN_MV), 3, 2)))
                vx, vy = M.fragment_vectors(geo, pix, ms["mv"], ms["bmv"])
                vx, vy = np.where(kind >= 2, vx, 0), np.where(kind >= 2, -vy, 0)
                for p, g in enumerate(geo.planes):
                    sl = slice(g["froffset"], g["froffset"] + g["nfrags"])
                    top = lambda a: a[sl].reshape(g["nvfrags"], g["nhfrags"])[::-1]
                    assert np.array_equal(got["kind"][p], top(kind)), (kind_of_clip, k, p)
                    assert np.array_equal(got["mv"][p][..., 0], top(vx)) and np.array_equal(got["mv"][p][..., 1], top(vy)), (kind_of_clip, k, p)
        finally:
            enc.close()
            dec.close()
    print("macro-block modes met:", dict(zip(M.MODE_NAMES, seen.tolist())))
    assert seen[M.MV_FOUR] > 0 and seen[M.MV] > 0 and seen[M.NOMV] + seen[M.INTRA] + seen[M.GOLDEN_NOMV] + seen[M.GOLDEN_MV] > 0, seen


def test_reference_made_stream(trace_env):
    """tests/golden/ref_qcif_q32.npz through a slot-trace context: the key frame is all intra; in every frame the maps add up to the
    trace, vectors sit on fragments with a reference only, and the dense outputs are the luma maps."""
    from theora_amd.decoder import Decoder
    hdr, packets, _, _ = refcmp.load_fixture()
    dec = Decoder(hdr)
    moved = 0
    for k, pkt in enumerate(packets[:8]):
        assert dec.packetin(pkt)[0] == 0
        t = dec.slot_trace()
        got = fr.frame_info(fr.from_trace(t, 176, 144, 0), 176, 144, 0, None, 3, np.float32)
        ncoded = sum(int((kd != 0).sum()) for kd in got["kind"])
        assert ncoded == t["fragi"].size and sum(int((kd == 0).sum()) for kd in got["kind"]) == t["uncoded"].size
        for kd, code in ((1, fr.FRAME_SELF), (2, fr.FRAME_PREV), (3, fr.FRAME_GOLD)):
            assert sum(int((m == kd).sum()) for m in got["kind"]) == int((t["refi"] == code).sum())
        assert sum(int(nc.astype(np.int64).sum()) for nc in got["ncoef"]) == int(t["last_zzi"].astype(np.int64).sum())
        if k == 0:
            assert t["frame_type"] == 0 and all((kd == 1).all() for kd in got["kind"])
        for p in range(3):
            assert not got["mv"][p][got["kind"][p] < 2].any()
        assert np.array_equal(got["valid"], np.kron(got["kind"][0], np.ones((8, 8), np.uint8)))
        assert np.array_equal(got["flow"][0], np.kron(got["mv"][0][..., 0] / np.float32(2), np.ones((8, 8), np.float32)))
        moved += int(got["flow"].any())
    assert moved >= 4        # (the clip moves: the encoder found vectors)
    dec.close()


@pytest.mark.parametrize("dx,dy", [(4, 0), (-3, 2), (0, -5)])
def test_planted_motion(trace_env, dx, dy):
    """The second frame is the first moved by (dx, dy) whole pixels, x to the right and y DOWN: cur(X, Y) = prev(X - dx, Y - dy).  By
    the defining property the predictor of (X, Y) is PREV at (X + vx / 2, Y + vy / 2), so the field is (-dx, -dy) wherever the
    content came from inside the frame."""
    from theora_amd.decoder import Decoder
    from theora_amd.encoder import Encoder
    w, h, q = 64, 48, 63
    e = Encoder(w, h, 0, q)
    hdr = e.header_packets()
    e.close()
    rng = np.random.default_rng(7)
    big = [rng.integers(16, 236, (h + 32, w + 32)).astype(np.uint8), np.full((h // 2 + 16, w // 2 + 16), 128, np.uint8),
           np.full((h // 2 + 16, w // 2 + 16), 128, np.uint8)]
    first = [big[0][16:16 + h, 16:16 + w], big[1][8:8 + h // 2, 8:8 + w // 2], big[2][8:8 + h // 2, 8:8 + w // 2]]
    second = [big[0][16 - dy:16 - dy + h, 16 - dx:16 - dx + w], first[1], first[2]]
    enc = M.ModesEncoder(w, h, 0, (0, 0, w, h), enc_ref.SetupParams(hdr[2]), 64, 6)
    dec = Decoder(hdr)
    try:
        for planes in (first, second):
            r = enc.frame([np.ascontiguousarray(a) for a in planes], q)
            assert dec.packetin(r["packet"])[0] == 0
        got = fr.frame_info(fr.from_trace(dec.slot_trace(), w, h, 0), w, h, 0, None, fr.REF_PREV, np.float32)
    finally:
        enc.close()
        dec.close()
    inner = (slice(16, h - 16), slice(16, w - 16))          # macro blocks whose content was inside the first frame
    assert (got["valid"][inner] == 2).all()
    assert (got["flow"][0][inner] == -dx).all() and (got["flow"][1][inner] == -dy).all()


def test_kernel_body_on_the_host_stays_inside_its_arrays(tmp_path):
    """k_frame_info's and k_frame_info_keep's lanes run one by one on the host under AddressSanitizer and UBSan
    (tests/native/frame_info_host.cpp): no load leaves the frame's words, no store leaves its destination rectangle, every 16-byte
    store is aligned, and every output equals a plain loop over fragments and pixels.  Every rectangle of a 40 x 24 frame in three
    pixel formats with the row alignment, padding, element type and source going round from one rectangle to the next; and for
    40 x 24 and 136 x 72 every column range at every row alignment 0..15 in both element types, and every row range (the program's
    head says why that stands for every rectangle of the larger frame).  Seven processes side by side."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "frame_info_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unused",
           "-Wno-unknown-pragmas", "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "theora_amd", "csrc"),
           os.path.join(root, "tests", "native", "frame_info_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = [("0", "0"), ("0", "2"), ("0", "3"), ("1",), ("2", "0"), ("2", "2"), ("2", "3")]
    procs = [subprocess.Popen([exe, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for a in runs]
    # 40 x 24: 820 column ranges x 300 row ranges; the sweeps: ranges x 16 alignments x 2 element types + row ranges x 4
    want = {"0": 820 * 300, "1": 3 * (820 * 32 + 300 * 4), "2": 9316 * 32 + 2628 * 4}
    for a, p in zip(runs, procs):
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0 and out.startswith("ok: %d requests" % want[a[0]]), (a, out[-500:], err[-3000:])


def _req(**kw):
    from theora_amd import _lib
    r = _lib.FrameInfoReq()
    r.valid, r.valid_pitch = 0x1000, 4096           # never dereferenced: every case below is refused
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_frame_info_arguments_checked_without_a_state():
    from theora_amd import _lib
    L = _lib.load()
    good = _req()
    assert L.thip_frame_info_out(None, 1, None) == _lib.EFAULT
    assert L.thip_frame_info_out(None, 0, None) == _lib.OK
    assert L.thip_frame_info_out(C.byref(good), 0, None) == _lib.OK
    assert L.thip_frame_info_out(C.byref(good), -1, None) == _lib.EINVAL
    assert L.thip_frame_info_out(None, -1, None) == _lib.EINVAL
    assert L.thip_frame_info_out(C.byref(good), 1, None) == _lib.EFAULT       # a NULL state
    reqs = (_lib.FrameInfoReq * 10)(*([good] * 10))
    assert L.thip_frame_info_out(reqs, 10, None) == _lib.EFAULT
    assert L.thip_state_set_frame_info(None, 1) == _lib.EFAULT
    assert C.sizeof(_lib.FrameInfoReq) == 8 + 8 + 4 * 6 + 3 * (3 * 8 + 3 * 8) + 4 * 8      # (no padding: the header's layout)
    assert (_lib.FI_REF_PREV, _lib.FI_REF_GOLD) == (1, 2)


def test_decoder_requests_in_slot_trace_mode(trace_env):
    """TH_DECCTL_THIP_SET_FRAME_INFO / _FRAME_INFO_OUT: the request numbers, the struct's size, and a context without device state
    (TH_EINVAL for the switch like the other device switches, TH_EIMPL for the output like the picture requests)."""
    from theora_amd import _lib
    from theora_amd import decoder as D
    assert (D.TH_DECCTL_THIP_SET_FRAME_INFO, D.TH_DECCTL_THIP_FRAME_INFO_OUT) == (0x710B, 0x710C)
    assert C.sizeof(D.FrameInfoArgs) == 4 * 8 + 3 * (3 * 8 + 3 * 8) + 4 * 8 + 8 + 4 * 6
    st = streamgen.Stream(32, 32, 0, seed=1)
    dec = D.Decoder(st.header_packets())
    a, v = D.FrameInfoArgs(), C.c_int(1)
    assert dec.ctl(D.TH_DECCTL_THIP_SET_FRAME_INFO, v, C.sizeof(v)) == _lib.EINVAL
    assert dec.ctl(D.TH_DECCTL_THIP_SET_FRAME_INFO, v, 2) == _lib.EINVAL
    assert dec.ctl(D.TH_DECCTL_THIP_SET_FRAME_INFO, None, 4) == _lib.EFAULT
    assert dec.ctl(D.TH_DECCTL_THIP_FRAME_INFO_OUT, a, C.sizeof(a)) == _lib.EIMPL
    assert dec.ctl(D.TH_DECCTL_THIP_FRAME_INFO_OUT, a, C.sizeof(a) - 8) == _lib.EINVAL
    assert dec.ctl(D.TH_DECCTL_THIP_FRAME_INFO_OUT, None, C.sizeof(a)) == _lib.EFAULT
    dec.close()
