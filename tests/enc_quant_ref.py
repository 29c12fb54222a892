"""enc_quant_ref.py -- TEST INFRASTRUCTURE: th_encode_*'s quantisation parameters (include/theoraenc_hip.h, "Quantisation
parameters") restated from the rules of that comment: the validity of a parameter set, the quantiser part of the setup header as
libtheora packs it, every step (spec 6.4.3), the rate probe's floor, and the parameter families the tests run under -- each unlike
the built-in set.  Pure numpy, no library."""
import os

import numpy as np

from tests import enc_ref

PAIRS = [(qti, pli) for qti in range(2) for pli in range(3)]


class Params:
    """dc, ac (64 scales each), lf (64 limits), sizes[qti][pli] (list of ints), mats[qti][pli] ((n + 1, 64) int64, natural order)."""

    def __init__(self, dc, ac, lf, sizes, mats):
        self.dc, self.ac, self.lf = [int(v) for v in dc], [int(v) for v in ac], [int(v) for v in lf]
        self.sizes = [[[int(v) for v in sizes[t][p]] for p in range(3)] for t in range(2)]
        self.mats = [[np.asarray(mats[t][p], np.int64).reshape(-1, 64) for p in range(3)] for t in range(2)]

    def copy(self):
        return Params(self.dc, self.ac, self.lf, self.sizes, [[m.copy() for m in row] for row in self.mats])

    def quant_info(self):
        from theora_amd.encoder import QuantInfo
        return QuantInfo(self.dc, self.ac, self.lf, self.sizes, self.mats)

    def same(self, qi):
        """Equal to a theora_amd.encoder.QuantInfo."""
        return qi == self.quant_info()


def valid(p):
    if any(v < 0 or v > 127 for v in p.lf):
        return False
    for t, pl in PAIRS:
        s = p.sizes[t][pl]
        if not 1 <= len(s) <= 63 or len(p.mats[t][pl]) != len(s) + 1 or any(v < 1 for v in s) or sum(s) != 63:
            return False
    return True


def consolidate(p):
    """-> (matrices, indices[qti][pli]): the distinct base matrices in first-seen order over (qti, pli, range end)."""
    bms, idx = [], [[None] * 3 for _ in range(2)]
    for t, pl in PAIRS:
        row = []
        for m in p.mats[t][pl]:
            for k, b in enumerate(bms):
                if np.array_equal(b, m):
                    row.append(k)
                    break
            else:
                bms.append(m)
                row.append(len(bms) - 1)
        idx[t][pl] = row
    return bms, idx


def _put(v, n):
    return format(int(v), "0%db" % n) if n else ""


def pack_bits(p):
    """The quantiser part of the setup header, a string of '0' and '1', and the code each of the five later (qti, pli) wrote
    ('01', '0', '00' or '1')."""
    ilog = enc_ref.ilog
    nb = max(ilog(v) for v in p.lf)
    out = [_put(nb, 3)] + [_put(v, nb) for v in p.lf]
    for sc in (p.ac, p.dc):
        nb = max(1, max(ilog(v) for v in sc))
        out += [_put(nb - 1, 4)] + [_put(v, nb) for v in sc]
    bms, idx = consolidate(p)
    out.append(_put(len(bms) - 1, 9))
    out += [_put(v, 8) for m in bms for v in m]
    bmbits = ilog(len(bms) - 1)
    ranges = [(p.sizes[t][pl], idx[t][pl]) for t, pl in PAIRS]
    codes = []
    for i, (t, pl) in enumerate(PAIRS):
        if i > 0:
            if t > 0 and ranges[i] == ranges[i - 3]:
                codes.append("01")
            elif ranges[i] == ranges[i - 1]:
                codes.append("00" if t > 0 else "0")
            else:
                codes.append("1")
            out.append(codes[-1])
            if codes[-1] != "1":
                continue
        sizes, ix = ranges[i]
        out.append(_put(ix[0], bmbits))
        qi = 0
        for k, s in enumerate(sizes):
            out.append(_put(s - 1, ilog(62 - qi)))
            qi += s
            out.append(_put(ix[k + 1], bmbits))
    return "".join(out), codes


def packet_bits(pkt):
    return "".join(format(b, "08b") for b in bytes(pkt))


def setup_packet(p, tree_bits):
    """The whole setup header packet: the quantiser part, then the 80 trees as given (a string of '0' and '1')."""
    bits = packet_bits(b"\x82theora") + pack_bits(p)[0] + tree_bits
    bits += "0" * (-len(bits) % 8)
    return bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))


def quant_bits_of_packet(pkt):
    """(the quantiser part of a setup header packet, the rest up to the last tree's end) as strings of '0' and '1'."""
    sp = QuantReader(pkt)
    bits = packet_bits(pkt)
    return bits[56:sp.quant_end], bits[sp.quant_end:sp.bits_used]


class QuantReader(enc_ref.SetupParams):
    """enc_ref.SetupParams that also notes where the quantiser part ends."""

    def __init__(self, packet):
        super().__init__(packet)
        br = enc_ref.BitReader(packet)
        br.read(56)
        br.read(64 * br.read(3))
        br.read(64 * (br.read(4) + 1))
        br.read(64 * (br.read(4) + 1))
        nbms = br.read(9) + 1
        br.read(nbms * 64 * 8)
        for t, pl in PAIRS:
            if (t, pl) != (0, 0) and not br.read(1):
                if t > 0:
                    br.read(1)
                continue
            br.read(enc_ref.ilog(nbms - 1))
            qi = 0
            while qi < 63:
                qi += br.read(enc_ref.ilog(62 - qi)) + 1
                br.read(enc_ref.ilog(nbms - 1))
        self.quant_end = br.pos


def from_setup(sp):
    """enc_ref.SetupParams -> Params (each (qti, pli) with matrices of its own)."""
    sizes = [[list(sp.qr[(t, pl)][0]) for pl in range(3)] for t in range(2)]
    mats = [[np.array([sp.bms[k] for k in sp.qr[(t, pl)][1]], np.int64) for pl in range(3)] for t in range(2)]
    return Params(sp.dcscale, sp.acscale, sp.lflims, sizes, mats)


def qmat(p, qti, pli, qi):
    """spec 6.4.3: the 64 steps in natural order."""
    sizes, mats = p.sizes[qti][pli], p.mats[qti][pli]
    qri, start = 0, 0
    while qri < len(sizes) - 1 and qi > start + sizes[qri]:
        start += sizes[qri]
        qri += 1
    size = sizes[qri]
    end = start + size
    bm = (2 * (end - qi) * mats[qri] + 2 * (qi - start) * mats[qri + 1] + size) // (2 * size)
    scale = np.full(64, p.ac[qi], np.int64)
    scale[0] = p.dc[qi]
    qmin = np.full(64, 8 if qti == 0 else 16, np.int64)
    qmin[0] = 16 if qti == 0 else 32
    return np.maximum(qmin, np.minimum(scale * bm // 100 * 4, 4096))


def steps(p):
    """[6 tables][64 q][64 z] uint16, zig-zag order: the intra then the inter table of each plane (thip_enc_rate_req.steps)."""
    out = np.empty((6, 64, 64), np.uint16)
    for t in range(6):
        for q in range(64):
            out[t, q] = qmat(p, t // 3, t % 3, q)[enc_ref.ZIGZAG]
    return out


def floor(st):
    """rate_form_floor: [6][64 z], the least step over q."""
    return np.asarray(st).reshape(6, 64, 64).min(axis=1)


# ---- the families --------------------------------------------------------------------------------------------------------------------
def _matrix(a, b, c=0):
    r, col = np.mgrid[0:8, 0:8]
    return np.clip(a + b * (r + col) + c * (r * col) // 4, 1, 255).astype(np.int64).reshape(64)


def _builtin_scales():
    ac = [int(np.floor(400.0 * (10.0 / 400.0) ** (q / 63.0) + 0.5)) for q in range(64)]
    dc = [int(np.floor(200.0 * (10.0 / 200.0) ** (q / 63.0) + 0.5)) for q in range(64)]
    lf = [(31 * (63 - q) + 31) // 63 for q in range(64)]
    return dc, ac, lf


def ref_family():
    """The reference encoder's parameters, parsed from the setup header stored in tests/golden/ref_qcif_q32.npz."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_qcif_q32.npz"))
    n = [int(v) for v in g["lengths"][:3]]
    return from_setup(enc_ref.SetupParams(g["data"][n[0] + n[1]:n[0] + n[1] + n[2]].tobytes()))


def ref_setup_packet():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_qcif_q32.npz"))
    n = [int(v) for v in g["lengths"][:3]]
    return g["data"][n[0] + n[1]:n[0] + n[1] + n[2]].tobytes()


def ranges_family():
    """Per (qti, pli) three ranges of sizes (1, 31, 31) over four distinct matrices; all six differ: 24 matrices."""
    dc, ac, lf = _builtin_scales()
    sizes = [[[1, 31, 31] for _ in range(3)] for _ in range(2)]
    mats = [[np.array([_matrix(14 + 2 * (3 * t + pl) + 5 * k, 2 + pl + (k & 1) + t, (k + pl) % 3) for k in range(4)])
             for pl in range(3)] for t in range(2)]
    return Params(dc, ac, lf, sizes, mats)


def saw_family():
    """Scales that rise and fall with qi.  ac: 60 + 10 |((qi + 5) mod 14) - 7|, least (60) at qi 2, 16, 30, 44, 58 and 110 at qi
    63; dc: 80 + 10 |(qi mod 10) - 5| but 60 at qi 0 alone, so the least DC step is at q = 0 only.  The built-in matrices, with the
    inter one made coarser (24 + 3 (r + c)); loop-filter limits that rise and fall too."""
    ac = [60 + 10 * abs((q + 5) % 14 - 7) for q in range(64)]
    dc = [60] + [80 + 10 * abs(q % 10 - 5) for q in range(1, 64)]
    lf = [3 + (5 * q) % 23 for q in range(64)]
    sizes = [[[63] for _ in range(3)] for _ in range(2)]
    m = [_matrix(16, 3, 1), _matrix(18, 5), _matrix(24, 3)]
    mats = [[np.array([m[pl if t == 0 and pl < 2 else (1 if t == 0 else 2)]] * 2) for pl in range(3)] for t in range(2)]
    return Params(dc, ac, lf, sizes, mats)


def shared_family(variant=False):
    """One matrix and one range for all six: one base matrix, indices of 0 bits, the codes '0', '0', '01', '01', '01'.  The variant
    has a second matrix for everything but intra luma: '1', '0', '00', '01', '01'."""
    dc, ac, lf = _builtin_scales()
    a, b = _matrix(16, 3), _matrix(20, 4)
    sizes = [[[63] for _ in range(3)] for _ in range(2)]
    mats = [[np.array([b if variant and (t, pl) != (0, 0) else a] * 2) for pl in range(3)] for t in range(2)]
    return Params(dc, ac, lf, sizes, mats)


def edge_family(high):
    """63 ranges of size 1 for one plane (64 distinct matrices), the others one range.  high = False: AC scales all 1, DC scales
    all 65535, limits all 0, the 63 ranges on intra luma; high = True: AC 65535, DC 1, limits all 127, the ranges on inter Cr."""
    sizes = [[[63] for _ in range(3)] for _ in range(2)]
    mats = [[np.array([_matrix(16 + 3 * t + pl, 2 + pl)] * 2) for pl in range(3)] for t in range(2)]
    t, pl = (1, 2) if high else (0, 0)
    sizes[t][pl] = [1] * 63
    mats[t][pl] = np.array([_matrix(10 + k, 1 + k % 5, k % 3) for k in range(64)])
    return Params([1 if high else 65535] * 64, [65535 if high else 1] * 64, [127 if high else 0] * 64, sizes, mats)


def families():
    return {"ref": ref_family(), "ranges": ranges_family(), "saw": saw_family(), "shared": shared_family(),
            "shared-variant": shared_family(True), "edge-low": edge_family(False), "edge-high": edge_family(True)}
