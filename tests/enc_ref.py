"""enc_ref.py -- TEST INFRASTRUCTURE: a restatement of the intra-only encoder's bitstream (include/theoraenc_hip.h, "The bitstream")
in numpy, to compare the library's packets with byte for byte.

The transform and quantiser are the oracle's (fdct8x8_batch, quantize_batch), coded order is the oracle's State.sb_order, the tokens
come from streamgen (value_token, eob_token, BitWriter).  The quantiser parameters and the Huffman trees are read back from the
encoder's own setup header by the small parser below: what is restated is how the encoder USES them.
"""
import numpy as np

import oracle
from tests.streamgen import BitWriter, eob_token, value_token
from theora_amd import synth

ZIGZAG = np.asarray(synth.FZIG_ZAG)


class BitReader:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8))
        self.pos = 0

    def read(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | int(self.bits[self.pos])
            self.pos += 1
        return v


def ilog(v):
    return int(v).bit_length()


class SetupParams:
    """Spec 6.4, read from a setup header packet."""

    def __init__(self, packet):
        br = BitReader(packet)
        assert br.read(8) == 0x82 and bytes(br.read(8) for _ in range(6)) == b"theora"
        nb = br.read(3)
        self.lflims = [br.read(nb) for _ in range(64)]
        nb = br.read(4) + 1
        self.acscale = [br.read(nb) for _ in range(64)]
        nb = br.read(4) + 1
        self.dcscale = [br.read(nb) for _ in range(64)]
        nbms = br.read(9) + 1
        self.bms = [np.array([br.read(8) for _ in range(64)], np.int64) for _ in range(nbms)]
        self.qr = {}
        for qti in range(2):
            for pli in range(3):
                newqr = 1 if (qti == 0 and pli == 0) else br.read(1)
                if not newqr:
                    rpqr = br.read(1) if qti > 0 else 0
                    self.qr[(qti, pli)] = self.qr[(qti - 1, pli)] if rpqr else self.qr[((3 * qti + pli - 1) // 3, (pli + 2) % 3)]
                    continue
                bmis, sizes, qi = [br.read(ilog(nbms - 1))], [], 0
                while qi < 63:
                    sizes.append(br.read(ilog(62 - qi)) + 1)
                    qi += sizes[-1]
                    bmis.append(br.read(ilog(nbms - 1)))
                assert qi == 63
                self.qr[(qti, pli)] = (sizes, bmis)
        self.codes = []   # per tree: token -> bit string
        for _ in range(80):
            codes = {}

            def rec(prefix, depth):
                assert depth <= 32
                if br.read(1):
                    codes[br.read(5)] = prefix
                else:
                    rec(prefix + "0", depth + 1)
                    rec(prefix + "1", depth + 1)
            rec("", 0)
            self.codes.append(codes)
        self.bits_used = br.pos

    def qmat(self, qti, pli, qi):
        """spec 6.4.3, natural order."""
        sizes, bmis = self.qr[(qti, pli)]
        qri, start = 0, 0
        while qri < len(sizes) - 1 and qi > start + sizes[qri]:
            start += sizes[qri]
            qri += 1
        size = sizes[qri]
        end = start + size
        bmi, bmj = self.bms[bmis[qri]], self.bms[bmis[qri + 1]]
        bm = (2 * (end - qi) * bmi + 2 * (qi - start) * bmj + size) // (2 * size)
        out = np.empty(64, np.int64)
        for ci in range(64):
            qmin = (16 if qti == 0 else 32) if ci == 0 else (8 if qti == 0 else 16)
            qscale = self.dcscale[qi] if ci == 0 else self.acscale[qi]
            out[ci] = max(qmin, min((qscale * int(bm[ci]) // 100) * 4, 4096))
        return out


def chroma_region(info_pic, fmt, pli):
    """(x0, y0, w, h) of the picture region in plane pli (spec 4.4), rows from the top."""
    x, y, w, h = info_pic
    hd = int(not (fmt & 1)) if pli else 0
    vd = int(not (fmt & 2)) if pli else 0
    x0, y0 = x >> hd, y >> vd
    return x0, y0, ((x + w + hd) >> hd) - x0, ((y + h + vd) >> vd) - y0


def frame_planes(planes, fw, fh, fmt, pic):
    """The three planes of the frame the encoder transforms (rows from the top): the picture, clamped outward."""
    st = oracle.State(fw, fh, fmt)
    out = []
    for p in range(3):
        g = st.planes[p]
        W, H = g["width"], g["height"]
        x0, y0, cw, ch = chroma_region(pic, fmt, p)
        a = np.asarray(planes[p], np.uint8)
        if a.shape == (H, W) and (cw, ch) != (W, H):
            a = a[y0:y0 + ch, x0:x0 + cw]
        assert a.shape == (ch, cw), (a.shape, ch, cw)
        rows = np.clip(np.arange(H) - y0, 0, ch - 1)
        cols = np.clip(np.arange(W) - x0, 0, cw - 1)
        out.append(a[rows][:, cols])
    st.close()
    return out


def dc_predict(dc, nh, nv):
    """Spec 7.8 on one plane's quantised DCs (raster, row 0 at the bottom), every fragment coded: the residuals."""
    q = dc.reshape(nv, nh).astype(np.int64)
    res = np.empty_like(q)
    for fy in range(nv):
        for fx in range(nh):
            m, l, ul, u, ur = 0, 0, 0, 0, 0
            if fx > 0:
                m |= 1
                l = q[fy, fx - 1]
            if fy > 0:
                if fx > 0:
                    m |= 2
                    ul = q[fy - 1, fx - 1]
                m |= 4
                u = q[fy - 1, fx]
                if fx + 1 < nh:
                    m |= 8
                    ur = q[fy - 1, fx + 1]
            tdiv = lambda a, b: int(a / b) if a >= 0 else -int(-a / b)   # C division towards zero
            if m == 0:
                pred = 0
            elif m in (1, 3):
                pred = l
            elif m == 2:
                pred = ul
            elif m in (4, 6, 12):
                pred = u
            elif m == 5:
                pred = tdiv(l + u, 2)
            elif m == 8:
                pred = ur
            elif m in (9, 11, 13):
                pred = tdiv(75 * l + 53 * ur, 128)
            elif m == 10:
                pred = tdiv(ul + ur, 2)
            elif m == 14:
                pred = tdiv(3 * (ul + ur) + 10 * u, 16)
            else:
                pred = tdiv(29 * (l + u) - 26 * ul, 32)
                if abs(pred - u) > 128:
                    pred = u
                elif abs(pred - l) > 128:
                    pred = l
                elif abs(pred - ul) > 128:
                    pred = ul
            res[fy, fx] = q[fy, fx] - pred
    return res.reshape(-1)


def block_tokens(v):
    """Tokens of one block (zig-zag values, DC already the residual): [(start index, token, extra, nbits)]; an EOB is
    (z, 'EOB')."""
    out, nxt = [], 0
    for z in np.nonzero(v)[0]:
        z = int(z)
        a, g = int(v[z]), z - nxt
        s, aa = (1 if a < 0 else 0), abs(a)
        if aa == 1 and 1 <= g <= 17:
            if g <= 5:
                out.append((nxt, 22 + g, s, 1))
            elif g <= 9:
                out.append((nxt, 28, (s << 2) | (g - 6), 3))
            else:
                out.append((nxt, 29, (s << 3) | (g - 10), 4))
        elif aa in (2, 3) and 1 <= g <= 3:
            if g == 1:
                out.append((nxt, 30, (s << 1) | (aa - 2), 2))
            else:
                out.append((nxt, 31, (s << 2) | ((aa - 2) << 1) | (g - 2), 3))
        else:
            if g > 0:
                out.append((nxt, 7, g - 1, 3) if g <= 8 else (nxt, 8, g - 1, 6))
            t = value_token(a)
            out.append((z, t[0], t[1], t[2]))
        nxt = z + 1
    if nxt < 64:
        out.append((nxt, "EOB"))
    return out


def huff_group(z):
    return 0 if z == 0 else 1 if z <= 5 else 2 if z <= 14 else 3 if z <= 27 else 4


def encode_frame(planes, fw, fh, fmt, pic, qi, setup):
    """The packet of one frame and what went into it: dict(packet, levels [n,64] zig-zag in coded order, coded_order,
    dequant [3][64] zig-zag, huff, tokens, tokens_merged, words: the tokens before the merge in stream order, in the word format of
    thip_encode.h, list_len [64][3])."""
    fr = frame_planes(planes, fw, fh, fmt, pic)
    st = oracle.State(fw, fh, fmt)
    geo = [dict(st.planes[p]) for p in range(3)]
    order = [st.sb_order(p) for p in range(3)]
    st.close()
    levels_by_plane, dq = [], []
    for p in range(3):
        g = geo[p]
        nh, nv = g["nhfrags"], g["nvfrags"]
        up = np.flipud(fr[p]).astype(np.int16) - 128            # row 0 at the bottom (spec 2.2)
        blocks = up.reshape(nv, 8, nh, 8).transpose(0, 2, 1, 3).reshape(nv * nh, 64)   # raster fragment order
        qz = setup.qmat(0, p, qi)[ZIGZAG]
        dq.append(qz)
        q, _ = oracle.quantize_batch(oracle.fdct8x8_batch(blocks), qz.astype(np.uint16))
        levels_by_plane.append(q.astype(np.int64))
    coded = np.concatenate(order)
    froff = [geo[p]["froffset"] for p in range(3)]
    lev = np.concatenate(levels_by_plane)                         # by global raster index
    levels = lev[coded]
    # DC residuals, tokens per block
    vals = lev.copy()
    for p in range(3):
        g = geo[p]
        sl = slice(froff[p], froff[p] + g["nfrags"])
        vals[sl, 0] = dc_predict(lev[sl, 0], g["nhfrags"], g["nvfrags"])
    plane_of = np.concatenate([np.full(geo[p]["nfrags"], p) for p in range(3)])
    by_z = {}
    last_zzi = np.zeros(len(coded), np.uint8)   # where each block reads its final token (the reference's last_zzi)
    for k, fi in enumerate(coded):
        toks = block_tokens(vals[fi])
        last_zzi[k] = toks[-1][0]
        for t in toks:
            by_z.setdefault((t[0], int(plane_of[fi])), []).append(t[1:])
    ntok = sum(len(v) for v in by_z.values())
    words = np.array([(z << 16 | p << 22) | (0 if t[0] == "EOB" else t[0] | t[1] << 5)
                      for z in range(64) for p in range(3) for t in by_z.get((z, p), [])], np.uint32)
    list_len = np.array([[len(by_z.get((z, p), [])) for p in range(3)] for z in range(64)], np.int64)
    # merge EOB runs across lists and planes, pieces of at most 4095 placed in the list of their first EOB
    lists, run, rstart = {}, 0, None

    def flush():
        nonlocal run
        if run:
            t = eob_token(run)
            lists.setdefault(rstart, []).append(t)
            run = 0
    for z in range(64):
        for p in range(3):
            for t in by_z.get((z, p), []):
                if t[0] == "EOB":
                    if run == 0:
                        rstart = (z, p)
                    run += 1
                    if run == 4095:
                        flush()
                    continue
                flush()
                lists.setdefault((z, p), []).append(t)
    flush()
    nmerged = sum(len(v) for v in lists.values())
    # tables: least bits, ties to the lower index
    hist = np.zeros((5, 2, 32), np.int64)
    for (z, p), toks in lists.items():
        for t in toks:
            hist[huff_group(z), int(p > 0), t[0]] += 1
    lens = np.array([[len(setup.codes[h].get(t, "")) for t in range(32)] for h in range(80)], np.int64)
    hti = []
    for c in range(4):
        ac, ch = c >> 1, c & 1
        groups = range(1, 5) if ac else range(0, 1)
        cost = [sum(int(hist[hg, ch] @ lens[16 * hg + t]) for hg in groups) for t in range(16)]
        hti.append(int(np.argmin(cost)))
    bw = BitWriter()
    bw.write(0, 1)
    bw.write(0, 1)
    bw.write(qi, 6)
    bw.write(0, 1)
    bw.write(0, 3)
    for z in range(64):
        if z < 2:
            bw.write(hti[2 * z], 4)
            bw.write(hti[2 * z + 1], 4)
        for p in range(3):
            codes = setup.codes[16 * huff_group(z) + hti[(2 if z else 0) + int(p > 0)]]
            for tok, extra, nb in lists.get((z, p), []):
                bw.code(codes[tok])
                bw.write(extra, nb)
    return dict(packet=bw.bytes(), levels=levels, coded_order=coded, dequant=np.array(dq), huff=hti, tokens=ntok,
                tokens_merged=nmerged, last_zzi=last_zzi, plane_of=plane_of[coded], flimit=setup.lflims[qi], words=words,
                list_len=list_len)


def oracle_decode(ost, ref):
    """Decodes encode_frame's frame with the oracle (an intra frame, every fragment coded); the picture is then
    ost.get_plane(oracle.FRAME_PREV, pli)[::-1]."""
    coded, lev, pl = ref["coded_order"], ref["levels"], ref["plane_of"]
    dq = ref["dequant"][pl]                       # [n, 64] zig-zag steps
    coeffs = np.zeros((len(coded), 64), np.int16)
    coeffs[:, ZIGZAG] = (lev * dq).astype(np.int16)
    coeffs[:, 0] = lev[:, 0]                      # the DC goes in raw (un-predicted) and is dequantised with dc_quant
    ost.coded[:] = 1
    ost.refi[:] = 2
    ost.mvs[:] = 0
    ncoded = [int((pl == p).sum()) for p in range(3)]
    return ost.decode_frame(frame_type=0, coded_fragis=coded, ncoded=ncoded, coeffs=coeffs, last_zzi=ref["last_zzi"],
                            dc_quant=dq[:, 0].astype(np.uint16), uncoded_fragis=np.zeros(0, np.int64), flimit=ref["flimit"])


# ---- pictures ---------------------------------------------------------------------------------------------------------------
def plane_shapes(fw, fh, fmt, pic=None, picture_size=False):
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    if picture_size:
        return [chroma_region(pic, fmt, p)[3:1:-1] for p in range(3)]
    return [(fh, fw), (fh >> vd, fw >> hd), (fh >> vd, fw >> hd)]


def content(kind, shape, seed=0):
    """A uint8 plane: flat, gradient, noise, or a seeded 'natural' image (smooth blobs, edges, texture)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.full(shape, int(rng.integers(0, 256)), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "gradient":
        return np.clip(255 * (0.6 * xx / max(w - 1, 1) + 0.4 * yy / max(h - 1, 1)), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    assert kind == "natural"
    img = np.full(shape, 110.0)
    for _ in range(12):   # smooth blobs
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        r = rng.uniform(0.05, 0.35) * max(h, w)
        img += rng.uniform(-60, 60) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    for _ in range(6):    # edges: half-planes
        a = rng.uniform(0, np.pi)
        d = np.cos(a) * (xx - rng.uniform(0, w)) + np.sin(a) * (yy - rng.uniform(0, h))
        img += rng.uniform(-40, 40) * (d > 0)
    img += 8 * np.sin(xx * rng.uniform(0.3, 1.2)) * np.sin(yy * rng.uniform(0.3, 1.2))   # texture
    img += rng.normal(0, 3, shape)
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def picture(kind, fw, fh, fmt, pic=None, picture_size=False, seed=0):
    return [content(kind, s, seed + p) for p, s in enumerate(plane_shapes(fw, fh, fmt, pic, picture_size))]
