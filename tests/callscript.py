"""Call scripts for th_decode_*: one list of API calls run through the reference decoder and through ours, and the two transcripts
compared call by call (tests/test_gpu_call_scripts.py on the device, tests/test_call_scripts_cpu.py in slot-trace mode).

A libtheora program may seek, call th_decode_ctl between frames, hand in a dropped frame or ask for the same picture twice; the
stream-order loop packetin(N), ycbcr_out(N), packetin(N + 1) is only one of the orders it may use.  A script is a list of operations
on one stream (headers and a list of data packets); run() makes the calls on a `side` (an adapter around one decoder) and returns
the transcript; compare() reports the first difference of two transcripts; generate() draws scripts from a seed.

Nothing here needs a device or the reference library: the sides are given decoders that somebody else made."""
import ctypes as C
import time

import numpy as np

TH_EFAULT, TH_EINVAL, TH_EBADPACKET = -1, -10, -24
GET_PPLEVEL_MAX, SET_PPLEVEL, SET_GRANPOS, SET_STRIPE_CB = 1, 3, 5, 7
SETTLE_SECONDS = 0.03           # (announced packets of these sizes parse in microseconds: the time is the parser thread's wake-up)


# ---- the operations ---------------------------------------------------------------------------------------------------------------
def packet(i):
    """th_decode_packetin(data packet i): the next one, a key frame elsewhere (a seek), an inter packet out of order."""
    return ("packet", int(i))


def empty():
    """th_decode_packetin of a zero-byte packet: a dropped frame."""
    return ("empty",)


def out(k=1):
    """th_decode_ycbcr_out k times."""
    return ("out", int(k))


def granpos(g, size=8):
    """TH_DECCTL_SET_GRANPOS; size is buf_sz (8 is right)."""
    return ("granpos", int(g), int(size))


def pplevel(level):
    """TH_DECCTL_SET_PPLEVEL (0 .. 7; 8 is refused)."""
    return ("pplevel", int(level))


def stripe(on):
    """TH_DECCTL_SET_STRIPE_CB: a callback that records its calls, or none."""
    return ("stripe", bool(on))


def ppmax():
    return ("ppmax",)


def announce(*indices):
    """TH_DECCTL_THIP_PREFETCH_PACKET for the listed packets (ours alone: the reference side ignores it)."""
    return ("announce",) + tuple(int(i) for i in indices)


def settle():
    """Time for the parser threads to finish what was announced (ours alone)."""
    return ("settle",)


def intended_refusal(op):
    """The code a th_decode_ctl the script drew as refused must return; None for a call that must succeed."""
    if op[0] == "granpos" and (op[2] != 8 or op[1] < 0):
        return TH_EINVAL
    if op[0] == "pplevel" and not 0 <= op[1] <= 7:
        return TH_EINVAL
    return None


def show(script, upto=None):
    ops = script if upto is None else script[:upto + 1]
    return "\n".join("  %3d  %s(%s)" % (k, op[0], ", ".join(repr(a) for a in op[1:])) for k, op in enumerate(ops))


# ---- the sides --------------------------------------------------------------------------------------------------------------------
class _Plane(C.Structure):      # th_img_plane with the pointer as a number (rows are read by address: a stride may be negative)
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("stride", C.c_int), ("data", C.c_void_p)]


_STRIPE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int)


class _StripeCb(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("fn", _STRIPE_FN)]


class RefSide:
    """oracle.ref.RefDecoder."""
    ours = False

    def __init__(self, dec):
        self.dec = dec

    def packetin(self, data):
        return self.dec.packetin(data)

    def out(self):
        return self.dec.ycbcr_out()

    def ctl(self, req, obj, size):
        return self.dec.ctl(req, C.byref(obj), size)

    def before(self, k):
        pass


class OurSide:
    """theora_amd.decoder.Decoder on the device.  announcing=False drops the announcements; `counters` is a function that reads the
    library's counters: what it returned before every operation is kept in .seen (and once more after the last one)."""
    ours = True

    def __init__(self, dec, announcing=True, counters=None):
        self.dec, self.announcing, self.counters, self.seen = dec, announcing, counters, []

    def packetin(self, data):
        return self.dec.packetin_raw(data)

    def out(self):
        return self.dec.ycbcr_out()

    def ctl(self, req, obj, size):
        return self.dec.ctl(req, obj, size)

    def announce(self, data):
        if self.announcing:
            self.dec.prefetch(data)

    def settle(self):
        if self.announcing:
            time.sleep(SETTLE_SECONDS)

    def before(self, k):
        if self.counters is not None:
            self.seen.append(self.counters())


# ---- the runner -------------------------------------------------------------------------------------------------------------------
class _Stripes:
    """What a stripe callback saw during one th_decode_packetin: the row ranges (fragment rows of the luma plane, from the top,
    theoradec.h:58-77) and the picture put together from the rows each call declared ready (-1 where no call did)."""

    def __init__(self):
        self.ranges, self.picture = [], None

    def __call__(self, ctx, buf, y0, y1):
        planes = (_Plane * 3).from_address(buf)
        if self.picture is None:
            self.picture = [np.full((p.height, p.width), -1, np.int16) for p in planes]
        self.ranges.append((int(y0), int(y1)))
        for p, pic in zip(planes, self.picture):
            sh = int(p.height != planes[0].height)          # (chroma rows: half as many where the format halves them)
            for y in range(max(0, y0 * 8 >> sh), min(p.height, y1 * 8 >> sh)):
                pic[y] = np.frombuffer(C.string_at(p.data + y * p.stride, p.width), np.uint8)


def run(side, script, packets):
    """The calls of `script` on `side`; the transcript: one entry an operation --
    packet / empty: dict(rc, granpos, stripes=[(y0, y1)...], stripe_picture=three planes or None),
    out: dict(pictures=[three planes] * k), a ctl: dict(rc, value), announce / settle: None."""
    T = []
    watcher = [None]

    def on_stripe(ctx, buf, y0, y1):
        watcher[0](ctx, buf, y0, y1)
    cb = _STRIPE_FN(on_stripe)          # (alive as long as the side's decoder may call it: the caller closes the decoder before this goes)
    side._stripe_keep = cb
    for k, op in enumerate(script):
        side.before(k)
        kind = op[0]
        if kind in ("packet", "empty"):
            watcher[0] = _Stripes()
            rc, gp = side.packetin(packets[op[1]] if kind == "packet" else b"")
            T.append(dict(rc=int(rc), granpos=int(gp), stripes=watcher[0].ranges, stripe_picture=watcher[0].picture))
        elif kind == "out":
            T.append(dict(pictures=[side.out() for _ in range(op[1])]))
        elif kind == "granpos":
            v = C.c_int64(op[1])
            T.append(dict(rc=int(side.ctl(SET_GRANPOS, v, op[2])), value=None))
        elif kind == "pplevel":
            v = C.c_int(op[1])
            T.append(dict(rc=int(side.ctl(SET_PPLEVEL, v, C.sizeof(v))), value=None))
        elif kind == "ppmax":
            v = C.c_int(-1)
            T.append(dict(rc=int(side.ctl(GET_PPLEVEL_MAX, v, C.sizeof(v))), value=int(v.value)))
        elif kind == "stripe":
            s = _StripeCb(None, cb if op[1] else _STRIPE_FN())
            T.append(dict(rc=int(side.ctl(SET_STRIPE_CB, s, C.sizeof(s))), value=None))
        elif kind == "announce":
            if side.ours:
                for i in op[1:]:
                    side.announce(packets[i])
            T.append(None)
        elif kind == "settle":
            if side.ours:
                side.settle()
            T.append(None)
        else:
            raise ValueError(op)
    side.before(len(script))
    return T


def rows_covered(ranges):
    """The fragment rows a list of stripe ranges covers, each once however the ranges were cut."""
    rows = set()
    for y0, y1 in ranges:
        rows |= set(range(y0, y1))
    return sorted(rows)


def _first_pixel(a, b):
    for p in range(3):
        if a[p].shape != b[p].shape:
            return "plane %d: shapes %r and %r" % (p, a[p].shape, b[p].shape)
        if not np.array_equal(a[p], b[p]):
            ys, xs = np.nonzero(a[p] != b[p])
            return "plane %d: %d pixels differ, the first at (y %d, x %d): %d and %d" % (
                p, ys.size, ys[0], xs[0], a[p][ys[0], xs[0]], b[p][ys[0], xs[0]])
    return None


def compare(a, b, script, seed=None, quiet=False):
    """The first difference of two transcripts of `script` as (seed, operation index, what), None if there is none; the script up
    to that operation is printed, so that the failure can be replayed by hand.  Everything in an entry is compared.  Stripe
    ranges are compared as the rows they cover and the picture they declare ready: how a decoder cuts a frame into stripes is its
    own business (theoradec.h:58-77: "typically" an MCU; ours makes one call a frame), which rows it hands out and with which
    pixels is not."""
    def entry(x, y):
        if (x is None) != (y is None):
            return "one side made a call here, the other none"
        if x is None:
            return None
        if sorted(x) != sorted(y):
            return "the entries are of different kinds: %r and %r" % (sorted(x), sorted(y))
        if "pictures" in x:
            if len(x["pictures"]) != len(y["pictures"]):
                return "%d pictures and %d" % (len(x["pictures"]), len(y["pictures"]))
            for n, (p, q) in enumerate(zip(x["pictures"], y["pictures"])):
                d = _first_pixel(p, q)
                if d:
                    return "th_decode_ycbcr_out number %d: %s" % (n, d)
            return None
        if x["rc"] != y["rc"]:
            return "return code %d and %d" % (x["rc"], y["rc"])
        if "granpos" in x:
            if x["granpos"] != y["granpos"]:
                return "granule position %d (0x%x) and %d (0x%x)" % (x["granpos"], x["granpos"], y["granpos"], y["granpos"])
            if bool(x["stripes"]) != bool(y["stripes"]):
                return "stripe callback: %d calls and %d" % (len(x["stripes"]), len(y["stripes"]))
            if rows_covered(x["stripes"]) != rows_covered(y["stripes"]):
                return "stripe callback: ranges %r and %r cover different rows" % (x["stripes"], y["stripes"])
            if x["stripe_picture"] is not None:
                d = _first_pixel(x["stripe_picture"], y["stripe_picture"])
                if d:
                    return "the picture the stripe callbacks declared ready: " + d
        elif x["value"] != y["value"]:
            return "value %r and %r" % (x["value"], y["value"])
        return None
    what, k = None, -1
    if len(a) != len(b) or len(a) != len(script):
        what, k = "%d and %d entries for %d operations" % (len(a), len(b), len(script)), min(len(a), len(b), len(script)) - 1
    else:
        for k in range(len(script)):
            what = entry(a[k], b[k])
            if what:
                break
    if not what:
        return None
    if not quiet:
        print("call script%s: first difference at operation %d: %s\n%s" % ("" if seed is None else " of seed %r" % (seed,), k, what,
                                                                          show(script, k)))
    return (seed, k, what)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
FORCED_CTLS = ("granpos_legal", "granpos_refused", "pplevel_key", "stripe_on")
FORCED_FOLLOWERS = ("announced", "other_key", "empty_then_announced")
DEFAULT_WEIGHTS = dict(next=8, seek=2, out_of_order=1, empty=2, out=5, granpos=2, granpos_refused=1, pplevel=3, stripe=2, ppmax=1,
                       announce_next=4, announce_other=1, settle=1)


def generate(seed, npackets, key_packets, nops=48, weights=None, ctls=True, shift=6):
    """A script of about `nops` operations from numpy.random.default_rng(seed).  key_packets: the indices of the key-frame packets
    (more than two, the first of them 0, none of the stream's packets empty); shift: the stream's keyframe_granule_shift (legal
    granule positions are drawn with an offset below 1 << shift); weights: of the random operations (DEFAULT_WEIGHTS); ctls=False
    leaves out pplevel and stripe (slot-trace mode has neither).

    Returns (script, forced): the script holds, between its random operations, one forced pattern for every entry of FORCED_CTLS
    (the two of granpos only with ctls=False) --
        [pplevel(0)] [stripe(off)] packet(c)  announce(c + 1, c + 2)  settle  out(1)  <the ctl>  <the follower>  out(1)
    -- the state in which th_decode_ycbcr_out has decoded packet c + 1 ahead: post-processing and stripe callback off, a frame
    decoded, nothing else announced (packet(c) is none of the packets that may still be announced, which drops them).  The
    follower is FORCED_FOLLOWERS in turn, starting at seed % 3 so that eight seeds meet every pair.  forced is the list of
    (index of the pattern's out(1), index of its ctl, ctl kind, follower kind)."""
    rng = np.random.default_rng(seed)
    keys = sorted(int(k) for k in key_packets)
    assert len(keys) > 2 and keys[0] == 0 and npackets >= 8
    w = dict(DEFAULT_WEIGHTS)
    w.update(weights or {})
    if not ctls:
        w["pplevel"] = w["stripe"] = 0
    names = [n for n in w if w[n] > 0]
    prob = np.array([w[n] for n in names], float)
    prob /= prob.sum()
    kinds = [c for c in FORCED_CTLS if ctls or c.startswith("granpos")]
    script, forced = [packet(0), out(1)], []
    st = dict(cur=0, pp=0, stripe=False, maybe=set())        # maybe: packets that may still be announced

    def handed(i):
        st["cur"] = i
        if i not in st["maybe"]:
            st["maybe"].clear()                              # (certainly not the oldest announcement: all of them are dropped)

    def legal_granpos():
        return 0 if rng.random() < 0.1 else (int(rng.integers(0, 1 << 20)) << shift) + int(rng.integers(0, 1 << shift))

    def refused_granpos():
        return granpos(-int(rng.integers(1, 1 << 40))) if rng.random() < 0.5 else granpos(legal_granpos(), size=int(rng.choice([0, 4, 16])))

    def random_op():
        n = names[int(rng.choice(len(names), p=prob))]
        nxt = st["cur"] + 1 if st["cur"] + 1 < npackets else int(rng.choice(keys))
        if n == "next":
            handed(nxt)
            return packet(nxt)
        if n == "seek":
            k = int(rng.choice(keys))
            handed(k)
            return packet(k)
        if n == "out_of_order":
            i = int(rng.integers(0, npackets))
            handed(i)
            return packet(i)
        if n == "empty":
            return empty()
        if n == "out":
            return out(int(rng.integers(0, 3)))
        if n == "granpos":
            return granpos(legal_granpos())
        if n == "granpos_refused":
            return refused_granpos()
        if n == "pplevel":
            lvl = int(rng.integers(0, 9))
            if lvl <= 7:
                st["pp"] = lvl
            return pplevel(lvl)
        if n == "stripe":
            st["stripe"] = bool(rng.integers(0, 2))
            return stripe(st["stripe"])
        if n == "ppmax":
            return ppmax()
        if n == "announce_next":
            ids = [i for i in (nxt, nxt + 1) if i < npackets][:int(rng.integers(1, 3))]
            st["maybe"].update(ids)
            return announce(*ids)
        if n == "announce_other":
            ids = [int(i) for i in rng.integers(0, npackets, int(rng.integers(1, 3)))]
            st["maybe"].update(ids)
            return announce(*ids)
        return settle()

    def forced_pattern(n):
        kind, follower = kinds[n % len(kinds)], FORCED_FOLLOWERS[(n + seed) % 3]
        if st["pp"]:
            script.append(pplevel(0))
            st["pp"] = 0
        if st["stripe"]:
            script.append(stripe(False))
            st["stripe"] = False
        # c + 1 and c + 2 exist, c + 1 is a key frame where the pattern asks for one, and c is not announced
        if kind == "pplevel_key":
            cs = [k - 1 for k in keys if k >= 1 and k + 1 < npackets]
        else:
            cs = list(range(0, npackets - 2))
        cs = [c for c in cs if c not in st["maybe"]] or cs
        c = int(rng.choice(cs))
        if c in st["maybe"]:                                 # (every candidate may be announced: one packet that is not, first)
            flush = next(i for i in range(npackets) if i not in st["maybe"] and i != c)
            script.append(packet(flush))
            handed(flush)
            st["maybe"].clear()
        script.append(packet(c))
        handed(c)
        st["maybe"].clear()
        script.extend([announce(c + 1, c + 2), settle(), out(1)])
        i_out = len(script) - 1
        if kind == "granpos_legal":
            script.append(granpos(legal_granpos()))
        elif kind == "granpos_refused":
            script.append(refused_granpos())
        elif kind == "pplevel_key":
            st["pp"] = int(rng.integers(2, 8))
            script.append(pplevel(st["pp"]))
        else:
            st["stripe"] = True
            script.append(stripe(True))
        forced.append((i_out, len(script) - 1, kind, follower))
        st["maybe"].update((c + 2,))
        if follower == "other_key":
            k = int(rng.choice([k for k in keys if k != c + 1]))
            script.append(packet(k))
            handed(k)
        else:
            if follower == "empty_then_announced":
                script.append(empty())
            script.append(packet(c + 1))
            handed(c + 1)
        script.append(out(1))

    nforced = len(kinds)
    nrandom = max(nforced + 1, nops - 2 - 9 * nforced)
    gaps = [nrandom // (nforced + 1) + (1 if g < nrandom % (nforced + 1) else 0) for g in range(nforced + 1)]
    for g in range(nforced + 1):
        for _ in range(gaps[g]):
            script.append(random_op())
        if g < nforced:
            forced_pattern(g)
    return script, forced


# ---- the streams ------------------------------------------------------------------------------------------------------------------
STREAMS = {   # name: (width, height, pixel format, picture region, key-frame interval, frames, quality): the smallest sizes at
    # which every plane still has partial super blocks; short intervals, so that a key frame often follows an announcement, and a
    # different keyframe_granule_shift each; a quality at which the post-processing filters change pixels
    "420": (64, 48, 0, (3, 5, 53, 37), 4, 24, 20),
    "422": (80, 48, 2, None, 5, 24, 20),
    "444": (48, 64, 3, None, 3, 24, 20),
}
_MADE = {}


def stream(name):
    """dict(headers, packets, keys, shift, w, h, fmt) of a stream the reference encoder makes on the CPU, once a session."""
    if name not in _MADE:
        from tests import refcmp
        w, h, fmt, pic, kf, n, q = STREAMS[name]
        hdr, pk = refcmp.ref_encode(refcmp.moving("natural", w, h, fmt, n, 3), w, h, fmt, pic=pic, quality=q, kf_interval=kf)
        packets = [p for p, _ in pk]
        assert len(packets) == n and all(packets) and len(set(packets)) == n        # none dropped, no two alike
        keys = [i for i, p in enumerate(packets) if not p[0] & 0x40]
        shift = 0
        while (1 << shift) < kf:
            shift += 1
        assert 2 < len(keys) < n and keys[0] == 0
        _MADE[name] = dict(headers=hdr, packets=packets, keys=keys, shift=shift, w=w, h=h, fmt=fmt)
    return _MADE[name]


SEEDS = list(range(8))
GPU_NOPS = 48


def gpu_script(name, seed):
    """The random script of (stream, seed) that tests/test_gpu_call_scripts.py runs."""
    s = stream(name)
    return generate(1000 * (1 + list(STREAMS).index(name)) + seed, len(s["packets"]), s["keys"], nops=GPU_NOPS, shift=s["shift"])
