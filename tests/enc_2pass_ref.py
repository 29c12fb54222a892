"""enc_2pass_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s two-pass mode (include/theoraenc_hip.h, "Two-pass") in
Python integers: the pass file's codec, the count TH_ENCCTL_THIP_2PASS_IN(NULL) answers, the second pass's controller, and both
passes composed from tests/enc_rate_ref.py's probe and tests/enc_inter_ref.py's encoder (five modes), to compare the library's
records, choices and packets with exactly.
"""
import struct

import oracle
from tests import enc_inter_ref
from tests import enc_rate_ref as RR

MAGIC, VERSION = b"THP2", 1
HEADER_BYTES, RECORD_BYTES = 1084, 264
KEY, INTER, DUP, DROPPED = 0, 1, 2, 3
U32 = (1 << 32) - 1


class NotFormat(ValueError):
    """A bad magic or version (the library's TH_ENOTFORMAT)."""


class Truncated(ValueError):
    """Fewer bytes than a header or a whole number of records."""


# ---- the pass file ---------------------------------------------------------------------------------------------------------------
def fields_of(fw, fh, pic, fmt, fps, shift, inter):
    """The eleven u32 of the header that must be the context's."""
    return [fw, fh, pic[0], pic[1], pic[2], pic[3], fmt, fps[0], fps[1], shift, int(bool(inter))]


def pack_header(fields, frames=0, dups=0, tot=None):
    tot = tot or [[0] * 64, [0] * 64]
    return MAGIC + struct.pack("<I11I2I", VERSION, *fields, frames, dups) + struct.pack("<128Q", *(tot[0] + tot[1]))


def unpack_header(data):
    if len(data) >= 8 and (data[:4] != MAGIC or struct.unpack("<I", data[4:8])[0] != VERSION):
        raise NotFormat("not a pass file")
    if len(data) < HEADER_BYTES:
        raise Truncated("a header of %d bytes" % len(data))
    v = struct.unpack("<11I2I", data[8:60])
    tot = list(struct.unpack("<128Q", data[60:HEADER_BYTES]))
    return dict(fields=list(v[:11]), frames=v[11], dups=v[12], tot=[tot[:64], tot[64:]])


def pack_record(rtype, qi, bits, E):
    """E saturates at 2^32 - 1, and so do the bits."""
    return struct.pack("<BBHI64I", rtype, qi, 0, min(bits, U32), *[min(max(int(x), 0), U32) for x in E])


def unpack_record(data):
    if len(data) != RECORD_BYTES:
        raise Truncated("a record of %d bytes" % len(data))
    v = struct.unpack("<BBHI64I", data)
    return dict(type=v[0], qi=v[1], bits=v[3], E=list(v[4:]))


def rec_class(rtype, inter):
    """The sum a record's curve enters: its type for key and inter, a drop with the inter frames (the key frames with inter frames
    off), a duplicate none."""
    return rtype if rtype <= INTER else (1 if inter else 0) if rtype == DROPPED else None


def finish_header(fields, records):
    """The finished header of the records (dicts of unpack_record): counts and sums."""
    tot = [[0] * 64, [0] * 64]
    for r in records:
        c = rec_class(r["type"], fields[10])
        if c is not None:
            for q in range(64):
                tot[c][q] += r["E"][q]
    dups = sum(r["type"] == DUP for r in records)
    return pack_header(fields, len(records) - dups, dups, tot)


def parse(data):
    """A whole pass file -> (header, records)."""
    h = unpack_header(data)
    body = data[HEADER_BYTES:]
    if len(body) % RECORD_BYTES or len(body) // RECORD_BYTES != h["frames"] + h["dups"]:
        raise Truncated("%d bytes of records for %d packets" % (len(body), h["frames"] + h["dups"]))
    return h, [unpack_record(body[k:k + RECORD_BYTES]) for k in range(0, len(body), RECORD_BYTES)]


def wanted(have, header, n):
    """What TH_ENCCTL_THIP_2PASS_IN(NULL) answers with `have` bytes in, before frame n (counted with the duplicates); header: the
    parsed header once its bytes are in, else None."""
    if header is None:
        return HEADER_BYTES - have
    if n >= header["frames"] + header["dups"]:
        return 0
    return max(HEADER_BYTES + (n + 1) * RECORD_BYTES - have, 0)


# ---- the second pass's controller -----------------------------------------------------------------------------------------------
def _corr(c, A, est):
    return min(max((c + (A << 16) // max(est, 1)) // 2, 4096), 1 << 20)


class Controller2:
    """The controller of "Two-pass", step for step.  rule="scale" is the library's: the rest of the file's recorded curves scaled by
    fresh / recorded of the frames seen so far, per class and per q.  rule="halving" is the rule first proposed for it (a Q16 r per
    class, r = clamp((r + (A << 16) / max(Rec[qi], 1)) / 2, 4096, 2^20) after each packet, Future(q) = sum (Tot - Seen) r >> 16),
    kept so that DESIGN.md section 5.17's comparison of the two can be repeated; the library does not have it."""

    def __init__(self, bitrate, fps, header, rule="scale"):
        self.bitrate, self.fps, self.h, self.rule = bitrate, fps, header, rule
        self.N = header["frames"] + header["dups"]
        self.inter = header["fields"][10]
        self.c, self.r = [65536, 65536], [65536, 65536]
        self.seen, self.fresh = [[0] * 64, [0] * 64], [[0] * 64, [0] * 64]
        self.A = 0

    @property
    def T(self):
        return min(max(self.bitrate * self.fps[1] // self.fps[0], 32), 1 << 40)

    @property
    def B(self):
        return self.T * self.N

    def _rest(self, u, q):
        """Y_u(q): what the recorded curves leave of class u at q, scaled."""
        x = max(self.h["tot"][u][q] - self.seen[u][q], 0)
        if self.rule == "halving":
            return x * self.r[u] >> 16
        y = x if self.seen[u][q] == 0 else min(x * self.fresh[u][q] // self.seen[u][q], 1 << 62)
        return y * self.c[u] >> 16

    def choose(self, rec, E, key):
        """rec: the frame's record; E: the fresh probe; key: the type the frame is coded with -> qi."""
        self.cls = rec_class(rec["type"], self.inter)
        self.rec, self.E = rec["E"], [int(x) for x in E]
        if self.cls is not None:
            for q in range(64):
                self.seen[self.cls][q] += self.rec[q]
                self.fresh[self.cls][q] = min(self.fresh[self.cls][q] + self.E[q], 1 << 62)
        t = 0 if key else 1
        left = self.B - self.A
        self.cur = [self.E[q] * self.c[t] >> 16 for q in range(64)]
        self.fut = [self._rest(0, q) + self._rest(1, q) for q in range(64)]
        qi = max([q for q in range(64) if self.cur[q] + self.fut[q] <= left], default=0)
        self.left_recorded = sum(max(self.h["tot"][u][qi] - self.seen[u][qi], 0) for u in range(2))
        self.ratio = [(self.fresh[u][qi] << 16) // self.seen[u][qi] if self.seen[u][qi] else 65536 for u in range(2)]
        return qi

    def coded(self, key, qi, A):
        t = 0 if key else 1
        self.A += A
        self.c[t] = _corr(self.c[t], A, self.E[qi])
        if self.cls is not None and self.rule == "halving":
            self.r[self.cls] = _corr(self.r[self.cls], A, self.rec[qi])


class OnePass:
    """tests/enc_rate_ref.py's one-pass controller on planted curves, for comparison: choose(E, key, f, keypos) / coded."""

    def __init__(self, bitrate, fps, inter, K, shift, buffer=None):
        self.ctl = RR.Controller(bitrate, fps, inter, K, shift, flags=0, buffer=buffer)

    def choose(self, E, key, f, keypos):
        return self.ctl.choose(E, key, f, keypos, f == 0, keypos, 0)[0]

    def coded(self, key, qi, A):
        self.ctl.coded(key, qi, A)


# ---- content --------------------------------------------------------------------------------------------------------------------
def uneven_clip(n=24):
    """176 x 144, 4:2:0: the smooth pan for the first half, then the detailed composite of tests/test_encoder_mask_cpu.py moving by
    the pan's steps -- an easy half and a hard half."""
    from tests.test_encoder_mask_cpu import _composite, _shifted
    steps = [(0, 0), (3, 1), (4, -2), (1, 5), (-3, 3), (0, 0), (7, -1), (-5, -6), (2, 2), (9, 4)]
    out = enc_inter_ref.sequence("pan", 176, 144, 0, n // 2, seed=21)
    comp, x, y = _composite(), 0, 0
    for f in range(n - n // 2):
        x, y = x + steps[f % len(steps)][0], y + steps[f % len(steps)][1]
        out.append([a.copy() for a in _shifted(comp, x, y)])
    return out


# ---- the two passes, composed -----------------------------------------------------------------------------------------------------
class Pass1:
    """The first pass: frame(planes, dups) -> list of (packet, record bytes); file() -> the pass file.  Quality mode (quality=q:
    tests/enc_inter_ref.py's stream at that qi, every frame probed against the reference it is coded from) or bitrate mode
    (bitrate=b: tests/enc_rate_ref.py's stream, whose probe is the record's)."""

    def __init__(self, fw, fh, fmt, pic, setup, quality=None, bitrate=None, fps=(30, 1), inter=False, kf_interval=64, shift=6,
                 flags=RR.DROP_FRAMES | RR.CAP_OVERFLOW):
        self.fields = fields_of(fw, fh, pic, fmt, fps, shift, inter)
        self.quality, self.inter, self.K, self.shift = quality, inter, kf_interval, shift
        self.records = []
        if bitrate is not None:
            self.rs = RR.RateStream(fw, fh, fmt, pic, setup, bitrate, fps=fps, inter=inter, kf_interval=kf_interval, shift=shift,
                                    flags=flags)
            self.enc = self.rs.enc
        else:
            self.rs = None
            self.enc = enc_inter_ref.InterEncoder(fw, fh, fmt, pic, setup, kf_interval if inter else 1, shift)
            self.probe = RR.Probe(fw, fh, fmt, pic, setup)
        self.qi = 0

    def close(self):
        self.enc.close()

    def placeholder(self):
        return pack_header(self.fields)

    def frame(self, planes, dups=0):
        out = []
        if self.rs is not None:
            for pkt, rec in self.rs.frame(planes, dups):
                if rec.get("duplicate"):
                    out.append((pkt, pack_record(DUP, rec["qi"], 0, [0] * 64)))
                else:
                    rtype = DROPPED if rec["dropped"] else KEY if rec["key"] else INTER
                    out.append((pkt, pack_record(rtype, rec["qi"], 8 * len(pkt), rec["probe"])))
        else:
            e = self.enc
            off = e.cur + 1 - e.key
            key = e.key < 0 or off >= e.kf_interval or off + dups >= (1 << self.shift)
            if key:
                E = self.probe.key(planes)
            else:
                E = self.probe.inter(planes, [e.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)])
            r = e.frame(planes, self.quality, dups=dups)
            assert r["key"] == key
            out.append((r["packet"], pack_record(KEY if key else INTER, self.quality, 8 * len(r["packet"]), E)))
            out.extend((b"", pack_record(DUP, self.quality, 0, [0] * 64)) for _ in range(dups))
        self.records.extend(unpack_record(r) for _, r in out)
        return out

    def file(self):
        return finish_header(self.fields, self.records) + b"".join(pack_record(r["type"], r["qi"], r["bits"], r["E"])
                                                                   for r in self.records)


class Pass2:
    """The second pass over a pass file: frame(planes, dups) -> list of (packet, dict(qi, key, ...)), the frame's and then its
    duplicates'."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, passfile, fps=(30, 1), inter=False, shift=6, rule="scale"):
        self.header, self.records = parse(passfile)
        assert self.header["fields"] == fields_of(fw, fh, pic, fmt, fps, shift, inter)
        self.enc = enc_inter_ref.InterEncoder(fw, fh, fmt, pic, setup, 1 << shift, shift)
        self.probe = RR.Probe(fw, fh, fmt, pic, setup)
        self.ctl = Controller2(bitrate, fps, self.header, rule)
        self.inter, self.shift = inter, shift
        self.cur, self.key, self.qi = -1, -1, 0

    def close(self):
        self.enc.close()

    def frame(self, planes, dups=0):
        f = self.cur + 1
        rec = self.records[f]
        key = rec["type"] == KEY or not self.inter or self.key < 0 or f - self.key + dups >= (1 << self.shift)
        if key:
            E = self.probe.key(planes)
        else:
            E = self.probe.inter(planes, [self.enc.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)])
        qi = self.ctl.choose(rec, E, key)
        r = self.enc._key(planes, qi) if key else self.enc._inter(planes, qi)
        A = 8 * len(r["packet"])
        self.ctl.coded(key, qi, A)
        if key:
            self.key = f
        self.cur = f + dups
        self.qi = qi
        st = dict(qi=qi, key=int(key), probe=[int(x) for x in E], actual=A, corr=list(self.ctl.c), ratio=list(self.ctl.ratio),
                  budget_left=self.ctl.B - self.ctl.A, recorded_left=self.ctl.left_recorded, recorded=list(rec["E"]))
        return [(r["packet"], st)] + [(b"", dict(qi=qi, key=0, duplicate=1)) for _ in range(dups)]
