"""Shared by tests/test_reference_cpu.py and tests/test_gpu_reference.py: the reference codec (oracle/ref.py) on one side, the
oracle, the front end, the kernels and the encoder on the other.  Every comparison is integer and exact."""
import contextlib
import hashlib

import numpy as np
import pytest

import oracle
from oracle import ref

TALLY = dict(frames=0, planes=0, blocks=0)     # what the session compared, for the log


def need_ref():
    """The reference library.  Where the library or the reference tree is present it loads (built on demand; a failure to build
    or load is a failure of the test); where neither is, the test skips."""
    if not ref.available():
        pytest.skip("no oracle/_ref/libtheora_ref.so and no reference tree: __graft_entry__.build() makes the library where the "
                    "tree is")
    return ref.lib()


@contextlib.contextmanager
def trace_mode():
    """Decoder contexts allocated inside record the slot calls instead of running them (option fe_trace_backend): no device."""
    from theora_amd import _lib
    L = _lib.load()
    old = L.thip_option(b"fe_trace_backend")
    assert L.thip_set_option(b"fe_trace_backend", 1) == 0
    try:
        yield
    finally:
        L.thip_set_option(b"fe_trace_backend", old)


def oracle_apply_trace(ost, t):
    """One frame's recorded slot calls (Decoder.slot_trace()) -> the oracle."""
    ost.refi[:] = oracle.FRAME_NONE
    ost.refi[t["fragi"]] = t["refi"]
    ost.mvs[:] = 0
    ost.mvs[t["fragi"]] = t["mv"]
    ncoded = [int((t["pli"] == p).sum()) for p in range(3)]
    return ost.decode_frame(t["frame_type"], t["fragi"], ncoded, t["coeffs"], t["last_zzi"], t["dc_quant"], t["uncoded"], t["flimit"])


def oracle_picture(ost):
    """The frame the oracle just finished, rows top first like th_decode_ycbcr_out."""
    return [ost.get_plane(oracle.FRAME_PREV, p)[::-1] for p in range(3)]


def diff_planes(a, b):
    """[(plane, differing pixels, first y, first x)] of two pictures; empty when equal."""
    bad = []
    for p in range(3):
        if a[p].shape != b[p].shape:
            bad.append((p, -1, a[p].shape, b[p].shape))
        elif not np.array_equal(a[p], b[p]):
            ys, xs = np.nonzero(a[p] != b[p])
            bad.append((p, int(ys.size), int(ys[0]), int(xs[0])))
    TALLY["planes"] += 3
    return bad


def compare_stream(headers, packets, w, h, fmt, truth_inputs=None, alter=None):
    """The packets through the reference decoder, through theora_amd.decoder.Decoder in slot-trace mode with its slot calls fed to
    the oracle, and (truth_inputs: per packet None or a function ost -> oracle.State.decode_frame arguments, the generator's
    ground truth) straight into a second oracle.  Return codes and granule positions of the two packetin must agree; the pictures
    must agree plane for plane on every frame.  alter(frame index, kwargs or trace) may change the oracle's input (the teeth test).
    Returns the list of mismatches [(frame, which, detail)] and the reference's pictures."""
    from theora_amd.decoder import Decoder
    rd = ref.RefDecoder(headers)
    bad, pictures = [], []
    with trace_mode():
        dec = Decoder(headers)
        o_trace, o_truth = oracle.State(w, h, fmt), oracle.State(w, h, fmt)
        started = False
        for f, pkt in enumerate(packets):
            r_ref, r_own = rd.packetin(pkt), dec.packetin(pkt)
            if r_ref != r_own:
                bad.append((f, "packetin", (r_ref, r_own)))
            if r_ref[0] < 0:
                continue
            want = rd.ycbcr_out()
            pictures.append(want)
            if r_ref[0] == 0:
                started = True
                t = dec.slot_trace()
                if alter is not None:
                    alter(f, t)
                if oracle_apply_trace(o_trace, t) != 0:
                    bad.append((f, "oracle refused the front end's slot calls", None))
                TALLY["blocks"] += int(t["fragi"].size + t["uncoded"].size)
                if truth_inputs is not None and truth_inputs[f] is not None:
                    if o_truth.decode_frame(**truth_inputs[f](o_truth)) != 0:
                        bad.append((f, "oracle refused the ground truth", None))
            if not started:
                continue            # (a dropped frame before any frame: the grey dummy, which the oracle has no notion of)
            TALLY["frames"] += 1
            d = diff_planes(want, oracle_picture(o_trace))
            if d:
                bad.append((f, "front end -> oracle != reference", d))
            if truth_inputs is not None:
                d = diff_planes(want, oracle_picture(o_truth))
                if d:
                    bad.append((f, "ground truth -> oracle != reference", d))
        dec.close()
        o_trace.close()
        o_truth.close()
    rd.close()
    return bad, pictures


# ---- content ----------------------------------------------------------------------------------------------------------------------
def lcg_frames(w, h, fmt, n, temporal=False):
    """SURVEY.md section 8(d)'s deterministic generator: LCG s = s * 1664525 + 1013904223, rnd = s >> 16, seed 12345, one draw a luma
    pixel in raster order; moving gradient + moving checkerboard + noise (+-4, or +-32 with temporal=True)."""
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    # the LCG, vectorised: s_k = a^k s_0 + c (a^k - 1) / (a - 1) mod 2^32, built by doubling
    total = n * w * h
    a, c = np.uint64(1664525), np.uint64(1013904223)
    m = np.uint64(0xFFFFFFFF)
    s = np.empty(total, np.uint64)
    s[0] = (np.uint64(12345) * a + c) & m
    filled, ak, ck = 1, a, c                     # x -> ak * x + ck advances by `filled` steps
    while filled < total:
        k = min(filled, total - filled)
        s[filled:filled + k] = (s[:k] * ak + ck) & m
        ck = (ck * ak + ck) & m
        ak = (ak * ak) & m
        filled += k
    rnd = (s >> np.uint64(16)).astype(np.int64).reshape(n, h, w)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    cy, cx = np.mgrid[0:h >> vd, 0:w >> hd].astype(np.int64)
    out = []
    for f in range(n):
        noise = rnd[f] % 65 - 32 if temporal else rnd[f] % 9 - 4
        lum = (((x + 3 * f) * 255 // w + (2 * y + f) * 255 // h) // 2 + 40 * ((((x + 2 * f) >> 4) ^ (y >> 4)) & 1) + noise)
        out.append([np.clip(lum, 16, 235).astype(np.uint8), (128 + ((cx + f) & 63) - 32).astype(np.uint8),
                    (128 + ((cy - f) & 63) - 32).astype(np.uint8)])
    return out


def moving(kind, w, h, fmt, n, seed=0):
    """n frames of tests/enc_ref.py content that moves: a window sliding over a larger seeded picture, so that inter frames carry
    vectors and residuals."""
    from tests import enc_ref
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    big = [enc_ref.content(kind, (h + 64, w + 64), seed), enc_ref.content(kind, ((h + 64) >> vd, (w + 64) >> hd), seed + 1),
           enc_ref.content(kind, ((h + 64) >> vd, (w + 64) >> hd), seed + 2)]
    out = []
    for f in range(n):
        dx, dy = (3 * f) % 60, (2 * f) % 60
        out.append([np.ascontiguousarray(big[0][dy:dy + h, dx:dx + w]),
                    np.ascontiguousarray(big[1][dy >> vd:(dy >> vd) + (h >> vd), dx >> hd:(dx >> hd) + (w >> hd)]),
                    np.ascontiguousarray(big[2][dy >> vd:(dy >> vd) + (h >> vd), dx >> hd:(dx >> hd) + (w >> hd)])])
    return out


def ref_encode(frames, w, h, fmt=0, **kw):
    """(header packets, [(packet, granulepos)]) of the reference encoder over the frames."""
    e = ref.RefEncoder(w, h, fmt, **kw)
    hdr = e.header_packets()
    pk = []
    for k, fr in enumerate(frames):
        pk.extend(e.encode(fr, last=k == len(frames) - 1))
    e.close()
    return hdr, pk


def more_than_one_qi(pkt):
    """A data packet whose frame header lists more than one qi."""
    return len(pkt) > 1 and not (pkt[0] & 0x80) and bool(pkt[1] & 0x80)


def load_fixture():
    """tests/golden/ref_qcif_q32.npz: (header packets, data packets, granule positions, digests)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_qcif_q32.npz"))
    cuts = np.concatenate([[0], np.cumsum(g["lengths"])])
    pk = [g["data"][cuts[k]:cuts[k + 1]].tobytes() for k in range(len(g["lengths"]))]
    return pk[:3], pk[3:], [int(v) for v in g["granulepos"]], [str(d) for d in g["digests"]]


def digest(planes):
    return hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for p in planes)).hexdigest()


# ---- inputs of the block kernels ----------------------------------------------------------------------------------------------------
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


def idct_inputs(seed=0, per_class=3):
    """(coefficients [n,64] natural order, last_zzi [n]) for every last_zzi 0..64: only the first last_zzi zig-zag positions are
    non-zero, as the decoder guarantees.  Classes: small, typical dequantised, the full int16 range, and one +-32767 / -32768 at
    each position."""
    rng = np.random.default_rng(seed)
    xs, lz = [], []
    for last in range(65):
        for cls in range(3):
            for _ in range(per_class):
                z = np.zeros(64, np.int64)
                if cls == 0:
                    z[:last] = rng.integers(-3, 4, last)
                elif cls == 1:
                    z[:last] = rng.integers(-40, 41, last) * rng.integers(8, 120, last) * (rng.random(last) < 0.5)
                    if last:
                        z[0] = rng.integers(-2000, 2001)
                else:
                    z[:last] = rng.integers(-32768, 32768, last)
                x = np.zeros(64, np.int16)
                x[ZIGZAG] = np.clip(z, -32768, 32767)
                xs.append(x)
                lz.append(last)
    for pos in range(64):
        for v in (32767, -32767, -32768):
            x = np.zeros(64, np.int16)
            x[ZIGZAG[pos]] = v
            for last in {pos + 1, 64, 10 if pos < 10 else 64, 3 if pos < 3 else 64}:     # every branch of the transform that may see it
                xs.append(x)
                lz.append(last)
    return np.array(xs, np.int16), np.array(lz, np.int32)


def fdct_inputs(seed=0, n=600):
    """Residual blocks in [-255, 255]: random of several spreads, the four constant +-255 / +-1 blocks, checkerboards, stripes."""
    rng = np.random.default_rng(seed)
    xs = [rng.integers(-255, 256, 64) for _ in range(n // 3)]
    xs += [np.clip(np.round(rng.normal(0, s, 64)), -255, 255) for s in (1, 4, 20, 90) for _ in range(n // 6)]
    xs += [np.full(64, v) for v in (255, -255, 1, -1, 0, 128, -128)]
    i, j = np.mgrid[0:8, 0:8]
    for amp in (255, 1, 77):
        xs += [(amp * (1 - 2 * ((i + j) & 1))).reshape(-1), (-amp * (1 - 2 * ((i + j) & 1))).reshape(-1),
               (amp * (1 - 2 * (i & 1))).reshape(-1), (amp * (1 - 2 * (j & 1))).reshape(-1),
               (amp * (1 - 2 * ((i >> 1 ^ j >> 2) & 1))).reshape(-1)]
    for k in range(64):     # one sample at +-255 on a flat block
        x = np.zeros(64)
        x[k] = 255 if k & 1 else -255
        xs.append(x)
    return np.array(xs, np.int16)


def pixel_planes(seed=0, w=96, h=72):
    """Two uint8 planes for the SAD / SATD / SSD families: `src` with flat, gradient, noisy and saturated regions, `ref` = src moved
    and perturbed, so that small, large and zero differences all occur."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    src = (x * 3 + y * 2) % 256
    src[: h // 3] = rng.integers(0, 256, (h // 3, w))
    src[h // 3: h // 2, : w // 2] = 255
    src[h // 3: h // 2, w // 2:] = 0
    src = src.astype(np.uint8)
    ref_ = np.roll(src, (1, 2), (0, 1)).astype(np.int64) + rng.integers(-6, 7, (h, w)) * (rng.random((h, w)) < 0.5)
    ref_[h // 3: h // 2, : w // 4] = 0          # the largest differences a block can have
    ref_[-16:, :32] = src[-16:, :32]            # and none at all
    return src, np.clip(ref_, 0, 255).astype(np.uint8)


def block_offsets(seed, w, h, n):
    """n block positions (byte offsets) with 8 pixels of room to the right and below, and a second and third set near them."""
    rng = np.random.default_rng(seed + 1)
    xs, ys = rng.integers(0, w - 9, n), rng.integers(0, h - 9, n)
    so = ys * w + xs
    ro = np.clip(ys + rng.integers(-2, 3, n), 0, h - 9) * w + np.clip(xs + rng.integers(-2, 3, n), 0, w - 9)
    r2 = np.clip(ro + rng.choice([1, -1, w, -w, w + 1], n), 0, (h - 9) * w + w - 9)
    return so.astype(np.int32), ro.astype(np.int32), r2.astype(np.int32)


def quant_inputs(dequant_zz, rng, nrandom=6):
    """Coefficient blocks (zig-zag order) for one dequantisation table: at every position the values that sit exactly on, one below
    and one above each rounding threshold k * q +- q / 2 and each multiple k * q (both signs, k up to the int16 range's edge), and
    random ones."""
    q = dequant_zz.astype(np.int64)
    rows = []
    for k in (0, 1, 2, 3, 7, 50):
        for half in (0, 1):
            base = k * q + half * (q >> 1)
            for d in (-1, 0, 1):
                for s in (1, -1):
                    rows.append(np.clip(s * (base + d), -32768, 32767))
            if half:
                rows.append(np.clip(k * q + ((q + 1) >> 1), -32768, 32767))
    rows.append(np.full(64, 32767))
    rows.append(np.full(64, -32768))
    for _ in range(nrandom):
        rows.append(rng.integers(-600, 601, 64) * (rng.random(64) < 0.6))
        rows.append(rng.integers(-32768, 32768, 64))
    return np.array(rows, np.int16)


def pp_tables(setup):
    """pp_dc_scale and pp_sharp_mod from a setup header's parameters (tests/streamgen.Setup or tests/enc_ref.SetupParams), as the
    reference derives them when it unpacks the header: the DC scale from the last table it builds (inter, Cr), the sharpening
    modifier from four mid-frequency steps of all six tables."""
    dcs, shm = np.zeros(64, np.int32), np.zeros(64, np.int32)
    for qi in range(64):
        sizes, bmis = setup.qr[(1, 2)]
        qri, start = 0, 0
        while qri < len(sizes) - 1 and qi > start + sizes[qri]:
            start += sizes[qri]
            qri += 1
        size, end = sizes[qri], start + sizes[qri]
        base0 = (2 * (end - qi) * int(setup.bms[bmis[qri]][0]) + 2 * (qi - start) * int(setup.bms[bmis[qri + 1]][0]) + size) // (2 * size)
        dcs[qi] = setup.dcscale[qi] * base0 // 160
        qsum = 0
        for qti in range(2):
            for pli in range(3):
                zz = setup.qmat(qti, pli, qi)[ZIGZAG]
                qsum += int(zz[12] + zz[17] + zz[18] + zz[24]) << (1 if pli == 0 else 0)
        shm[qi] = -(qsum >> 11)
    return dcs, shm
