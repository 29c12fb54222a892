"""The arrays of thip_token_lists (include/theora_hip.h, "The whole step between the entropy decoder and the pixel path") built
from a theora_amd.synth frame, and the plain walk that reads them back: the reference of the operation the token-list kernels
perform.  Written from the header's text and the specification's section 7.7: a packer (numpy, per fragment), the per-fragment loop
of decode.c:1540-1581 (a few lines of Python, no parallelism), and helpers that edit a synth frame so that a test chooses the coded
counts and the shape of a list.  No device code and no oracle in here."""
import ctypes as C

import numpy as np

from theora_amd import FRAME_SELF, synth

TOK_EOB = 1 << 23


class TokenLists(C.Structure):
    """thip_token_lists (include/theora_hip.h)."""
    _fields_ = [("frame_type", C.c_int32), ("flimit", C.c_int32), ("tokens", C.c_void_p), ("ntokens", C.c_int64),
                ("list_off", C.c_uint32 * 64 * 3), ("list_len", C.c_uint32 * 64 * 3), ("eob_carry", C.c_uint32 * 64 * 3),
                ("arrivals", C.c_uint32 * 64 * 3), ("coded", C.c_void_p), ("frag_meta", C.c_void_p),
                ("ncoded", C.c_int32 * 3), ("dequant", C.c_void_p), ("dc_quant", C.c_uint16 * 2 * 3), ("dc", C.c_void_p)]


def table(a):
    """A [3][64] table of the packer as the C array the entry points take."""
    return (C.c_uint32 * 64 * 3).from_buffer_copy(np.ascontiguousarray(a, np.uint32).tobytes())


def as_struct(lists, dc=True):
    """pack()'s fields as a TokenLists; dc=False leaves `dc` NULL (the device undoes the prediction).  Returns (struct, keepalive)."""
    keep = dict(tokens=np.ascontiguousarray(lists["tokens"], np.uint32), coded=np.ascontiguousarray(lists["coded"], np.int32),
                frag_meta=np.ascontiguousarray(lists["frag_meta"], np.uint32), dequant=np.ascontiguousarray(lists["dequant"], np.uint16),
                dc=np.ascontiguousarray(lists["dc"], np.int16))
    tl = TokenLists()
    tl.frame_type, tl.flimit = int(lists["frame_type"]), int(lists["flimit"])
    tl.tokens, tl.ntokens = keep["tokens"].ctypes.data, int(keep["tokens"].size)
    for k in ("list_off", "list_len", "eob_carry", "arrivals"):
        setattr(tl, k, table(lists[k]))
    tl.coded, tl.frag_meta, tl.dequant = keep["coded"].ctypes.data, keep["frag_meta"].ctypes.data, keep["dequant"].ctypes.data
    for p in range(3):
        tl.ncoded[p] = int(lists["ncoded"][p])
        for q in range(2):
            tl.dc_quant[p][q] = int(lists["dc_quant"][p][q])
    tl.dc = keep["dc"].ctypes.data if dc else None
    return tl, keep


def pack(geom, frame, *, eob_cap, combine, dc_residual):
    """A synth frame as the fields of thip_token_lists.  eob_cap: the longest EOB run a token may carry (1, 4095, None: no cap);
    combine: a value with zeros before it is ONE token with the zeros in bits 16-22 (True) or a pure zero run followed by the value's
    own token (False); dc_residual: int16 per coded fragment, the value the token at index 0 carries (`dc` is the frame's un-predicted
    DC, coeffs[:, 0])."""
    cf = np.asarray(frame["coded_fragis"], np.int64)
    n = int(cf.size)
    ncoded = [int(x) for x in frame["ncoded"]]
    assert sum(ncoded) == n
    plane = np.repeat(np.arange(3), ncoded)
    refi = np.asarray(frame["refi"], np.int64)[cf]
    qti = (refi != FRAME_SELF).astype(np.int64)
    tab = (plane * 3 + np.asarray(frame["qii"], np.int64)) * 2 + qti
    meta = refi | tab << 2 | (np.asarray(frame["mvx"], np.int64)[cf] & 255) << 8 | (np.asarray(frame["mvy"], np.int64)[cf] & 255) << 16 | plane << 24
    dcq = np.zeros((3, 2), np.uint16)
    dcq[plane, qti] = np.asarray(frame["dc_quant"], np.uint16)
    assert np.array_equal(dcq[plane, qti], np.asarray(frame["dc_quant"], np.uint16))   # one dc_quant per (plane, qti)
    # ---- one event per token a fragment meets: (index it is met at, fragment, word) ---------------------------------------
    Z = np.asarray(frame["levels"], np.int16).reshape(-1, 64)[:, synth.FZIG_ZAG].astype(np.int64)   # zig-zag order
    Z[:, 0] = np.asarray(dc_residual, np.int64)
    f, k = np.nonzero(Z)                                      # fragment after fragment, positions rising
    first = np.ones(f.size, bool)
    first[1:] = f[1:] != f[:-1]
    start = np.where(first, 0, np.concatenate([[0], k[:-1] + 1])[:f.size])    # the index behind the fragment's previous value
    zeros = k - start
    val = Z[f, k] & 0xFFFF
    if combine:
        ez, ef, ew = [start], [f], [val | zeros << 16]
    else:
        run = zeros > 0
        ez, ef, ew = [start[run], k], [f[run], f], [zeros[run] << 16, val]
    last = np.full(n, -1, np.int64)
    np.maximum.at(last, f, k)
    ends = np.nonzero(last < 63)[0]                            # fragments that meet an EOB (token or run) behind their last value
    ez.append(last[ends] + 1)
    ef.append(ends)
    ew.append(np.full(ends.size, TOK_EOB, np.int64))
    ez, ef, ew = np.concatenate(ez), np.concatenate(ef), np.concatenate(ew)
    # the decoder's list order: index by index, planes 0, 1, 2 inside an index, fragments in coded order (`coded` is plane after plane)
    order = np.argsort(ez * max(n, 1) + ef, kind="stable")
    ez, ef, ew = ez[order], ef[order], ew[order]
    lid = plane[ef] * 64 + ez                                  # the list the event belongs to
    arrivals = np.bincount(lid, minlength=192).reshape(3, 64)
    # ---- EOB runs: consecutive ends merge, in pieces of at most eob_cap, the token in the list of the piece's first fragment ----
    N = int(ez.size)
    eob = ew == TOK_EOB
    idx = np.arange(N)
    run_start = eob.copy()
    run_start[1:] &= ~eob[:-1]
    at = idx - np.maximum.accumulate(np.where(run_start, idx, 0))   # place inside its run
    head = eob & (at % eob_cap == 0 if eob_cap else at == 0)
    keep = ~eob | head
    ki = np.nonzero(keep)[0]
    length = np.diff(np.concatenate([ki, [N]]))               # a head's run: up to the next token that stays
    words = ew[ki]
    kh = eob[ki]
    assert (length[~kh] == 1).all() and (length[kh] < 1 << 24).all()
    words[kh] = TOK_EOB | (length[kh] & 0xFFFF) | (length[kh] >> 16) << 24
    # the part of a run that reaches past its list: counted into the lists it reaches
    owner = ki[np.searchsorted(ki, idx, side="right") - 1]     # the token that ends this event's fragment
    past = ~keep & (lid != lid[owner])
    carry = np.bincount(lid[past], minlength=192).reshape(3, 64)
    klid = lid[ki]
    list_len = np.bincount(klid, minlength=192).reshape(3, 64)
    # all lists concatenated: index after index, the planes inside (a group of indices is one piece of the array)
    off_zp = np.concatenate([[0], np.cumsum(list_len.T.reshape(-1))[:-1]]).reshape(64, 3)
    return dict(frame_type=int(frame["frame_type"]), flimit=int(frame["flimit"]), tokens=words.astype(np.uint32),
                list_off=off_zp.T.astype(np.uint32).copy(), list_len=list_len.astype(np.uint32), eob_carry=carry.astype(np.uint32),
                arrivals=arrivals.astype(np.uint32), coded=cf.astype(np.int32), frag_meta=meta.astype(np.uint32), ncoded=ncoded,
                dequant=np.asarray(frame["dequant"], np.uint16).reshape(18, 64).copy(), dc_quant=dcq,
                dc=np.asarray(frame["coeffs"], np.int16).reshape(-1, 64)[:, 0].copy())


def group(lists, z0, z1):
    """The lists of the indices [z0, z1) as thip_state_token_lists_append takes them: (tokens, list_off counted from their start)."""
    lo = int(lists["list_off"][0][z0])
    hi = int(lists["list_off"][2][z1 - 1] + lists["list_len"][2][z1 - 1])
    off = lists["list_off"].astype(np.int64) - lo
    off[:, :z0] = 0
    off[:, z1:] = 0
    return np.ascontiguousarray(lists["tokens"][lo:hi]), off.astype(np.uint32)


def walk(lists):
    """decode.c:1540-1581 over the lists, fragment after fragment in coded order: a pending run ends the fragment, otherwise it takes
    the next token of list (plane, zzi).  Returns dict(levels [n][64] natural order with the DC token's value at 0, last_zzi [n],
    arrivals / used / carried [3][64]: the fragments seen arriving at an index, the tokens taken from its list, the fragments a run
    from an earlier list ended there)."""
    tok = np.asarray(lists["tokens"]).tolist()
    n = int(sum(lists["ncoded"]))
    last = np.zeros(n, np.uint8)
    rows, cols, vals = [], [], []
    seen, used, carried = np.zeros((3, 64), np.int64), np.zeros((3, 64), np.int64), np.zeros((3, 64), np.int64)
    c = 0
    for p in range(3):
        ti = np.asarray(lists["list_off"][p]).tolist()
        end = [a + b for a, b in zip(ti, np.asarray(lists["list_len"][p]).tolist())]
        first = list(ti)
        runs = np.asarray(lists["eob_carry"][p]).tolist()
        fresh, carr = [True] * 64, [0] * 64                  # no token of the list taken yet: what is pending is the carry
        arr = [0] * 64
        for _ in range(int(lists["ncoded"][p])):
            zzi = 0
            while zzi < 64:
                last_zzi = zzi
                arr[zzi] += 1
                if runs[zzi]:
                    runs[zzi] -= 1
                    carr[zzi] += fresh[zzi]
                    break
                fresh[zzi] = False
                assert ti[zzi] < end[zzi], "list (%d, %d) ran out" % (p, zzi)
                w = tok[ti[zzi]]
                ti[zzi] += 1
                if w & TOK_EOB:
                    runs[zzi] = ((w & 0xFFFF) | (w >> 24) << 16) - 1
                    break
                zzi += (w >> 16) & 127
                v = (w & 0xFFFF) - ((w & 0x8000) << 1)
                if v:
                    assert zzi < 64
                    rows.append(c)
                    cols.append(zzi)
                    vals.append(v)
                    zzi += 1
            last[c] = last_zzi
            c += 1
        seen[p] = arr
        used[p] = [a - b for a, b in zip(ti, first)]
        carried[p] = carr
    levels = np.zeros((n, 64), np.int16)
    if rows:
        levels[np.asarray(rows), synth.FZIG_ZAG[np.asarray(cols)]] = np.asarray(vals, np.int16)
    return dict(levels=levels, last_zzi=last, arrivals=seen, used=used, carried=carried)


# ---- helpers that edit a synth frame (in the manner of synth.nothing_coded and synth.widen_tiles) --------------------------------
def _copy(frame):
    return {k: v for k, v in frame.items() if not k.startswith("_")}   # (keys with an underscore: a caller's notes about THIS frame)


def _relevel(geom, frame, levels):
    out = _copy(frame)
    out["levels"] = levels
    out["coeffs"] = synth.dequantise(geom, out)
    return out


def with_coded(geom, frame, counts, rng):
    """The inter frame with exactly counts[p] coded fragments in plane p, scattered over the plane, the rest uncoded."""
    cf = np.asarray(frame["coded_fragis"], np.int64)
    base = np.concatenate([[0], np.cumsum(frame["ncoded"])])
    keep = np.zeros(cf.size, bool)
    for p in range(3):
        have = int(frame["ncoded"][p])
        assert 0 <= counts[p] <= have, (p, counts[p], have)
        keep[base[p] + np.sort(rng.choice(have, int(counts[p]), replace=False))] = True
    out = _copy(frame)
    refi = np.array(frame["refi"], np.uint8, copy=True)
    refi[cf[~keep]] = 3                                       # OC_FRAME_NONE, as synth.gen_frame marks the uncoded ones
    is_coded = np.zeros(geom.nfrags, bool)
    is_coded[cf[keep]] = True
    out.update(refi=refi, coded_fragis=cf[keep], ncoded=[int(c) for c in counts],
               uncoded_fragis=geom.coded_order[~is_coded[geom.coded_order]][::-1].copy())
    for k in ("coeffs", "levels", "last_zzi", "dc_quant", "qii", "dc_residual"):
        if k in frame:
            out[k] = np.asarray(frame[k])[keep]
    return out


def sparse(geom, frame, rng, p_ac, big=0.0):
    """Most blocks without AC levels (all-zero or DC-only, as the residual decides) and a share p_ac with one to three of them, so that
    a big frame carries about 1.3 tokens a fragment; a share `big` of those get a level beyond eight bits."""
    n = int(np.asarray(frame["coded_fragis"]).size)
    lv = np.zeros((n, 64), np.int16)
    lv[:, 0] = np.asarray(frame["levels"]).reshape(-1, 64)[:, 0]
    who = np.nonzero(rng.random(n) < p_ac)[0]
    for _ in range(3):
        w = who[rng.random(who.size) < 0.6]
        v = rng.integers(1, 10, w.size) * rng.choice([-1, 1], w.size)
        v = np.where(rng.random(w.size) < big, v * 40, v)
        lv[w, synth.FZIG_ZAG[rng.integers(1, 64, w.size)]] = v
    return _relevel(geom, frame, lv)


def residuals(frame, rng, p_zero=0.5):
    """A DC token value per coded fragment for frames whose `dc` the caller hands over: zero for a share p_zero (no token at index 0:
    the fragment starts with a zero run or ends there), small otherwise."""
    n = int(np.asarray(frame["coded_fragis"]).size)
    r = rng.integers(1, 200, n) * rng.choice([-1, 1], n)
    return np.where(rng.random(n) < p_zero, 0, r).astype(np.int16)


def shape_list(geom, frame, plane, z, m, rng):
    """The frame arranged so that list (plane, z) has exactly m tokens, whatever eob_cap and combine: m fragments of the plane,
    scattered, carry a value at index z that is met there (index z - 1 holds a value too, the DC residual for z == 1); every other
    fragment of the plane ends at index 0.  z == 0: the plane has m coded fragments (with_coded) and each has a residual.  The other
    planes stay as they are.  Sets frame["dc_residual"] (what pack's dc_residual is to be)."""
    nc = [int(x) for x in frame["ncoded"]]
    c0 = sum(nc[:plane])
    lv = np.array(frame["levels"], np.int16, copy=True).reshape(-1, 64)
    res = np.array(frame.get("dc_residual", np.zeros(lv.shape[0], np.int16)), np.int16, copy=True)
    lv[c0:c0 + nc[plane], 1:] = 0
    res[c0:c0 + nc[plane]] = 0
    if z == 0:
        assert nc[plane] == m
        who = c0 + np.arange(m)
    else:
        assert m <= nc[plane]
        who = c0 + np.sort(rng.choice(nc[plane], m, replace=False))
    val = lambda: (rng.integers(1, 100, m) * rng.choice([-1, 1], m)).astype(np.int16)
    if z <= 1:
        res[who] = val()
    else:
        lv[who, synth.FZIG_ZAG[z - 1]] = val()
    if z >= 1:
        lv[who, synth.FZIG_ZAG[z]] = val()
    out = _relevel(geom, frame, lv)
    out["dc_residual"] = res
    return out


def edge_frames(geom, frame, rng, share, names=None):
    """The list-shape edges of a frame, each a copy of `frame` (a sparse one with its "dc_residual") rearranged: name -> frame.
    share: the fragments a thread of the walking work group owns (32 x its groups), for the runs that end where a share does;
    names: only these."""
    nc = [int(x) for x in frame["ncoded"]]
    c0 = [0, nc[0], nc[0] + nc[1]]
    n = sum(nc)
    lv0 = np.asarray(frame["levels"], np.int16).reshape(-1, 64)
    res0 = np.asarray(frame["dc_residual"], np.int16)

    def make(edit):
        lv, res = lv0.copy(), res0.copy()
        edit(lv, res)
        out = _relevel(geom, frame, lv)
        out["dc_residual"] = res
        return out

    def end_at(lv, res, lo, hi, z):          # fragments lo..hi-1 (coded order) meet their end at index z: values at 0..z-1, nothing behind
        lv[lo:hi, 1:] = 0
        res[lo:hi] = 0
        if z >= 1:
            res[lo:hi] = 7
            lv[lo:hi, synth.FZIG_ZAG[1:z]] = -3

    def alive(lv, res, i):                   # fragment i takes a token at every index
        res[i] = -9
        lv[i, 1:] = 2 + (np.arange(63) % 5)

    def ended_at_0(lv, res):
        end_at(lv, res, 0, n, 0)

    def last_alive(lv, res):                 # only the plane's last fragment is open from index 1 on: one thread has arrivals
        end_at(lv, res, 0, nc[0], 0)
        alive(lv, res, nc[0] - 1)

    def carry_minus_1(lv, res):              # plane 1 at index 0: every arrival but the last ended by the run that comes over from plane 0
        end_at(lv, res, nc[0] - 10, nc[0], 0)
        end_at(lv, res, c0[1], c0[2], 0)
        alive(lv, res, c0[2] - 1)

    def run_to_plane_end(lv, res):           # a run over the last 40 fragments of plane 0, and plane 1 begins with a token
        alive(lv, res, nc[0] - 41)
        end_at(lv, res, nc[0] - 40, nc[0], 0)
        alive(lv, res, c0[1])

    def run_to_share_end(lv, res):           # runs that end on the last fragment of the first and of the last thread's share
        for hi in (share, ((nc[0] + share - 1) // share) * share):
            hi = min(hi, nc[0])
            alive(lv, res, hi - 13)
            end_at(lv, res, hi - 12, hi - 7, 2)
            end_at(lv, res, hi - 7, hi, 0)
            if hi < n:
                alive(lv, res, hi)

    def value_at_63(lv, res):                # a zero run that puts its value at the last index (met at 51, or at 63 behind a run token)
        who = np.nonzero(rng.random(n) < 0.3)[0]
        lv[who, 1:] = 0
        lv[who, synth.FZIG_ZAG[50]] = 5
        lv[who, synth.FZIG_ZAG[63]] = -4

    edits = [ended_at_0, last_alive, carry_minus_1, run_to_plane_end, run_to_share_end, value_at_63]
    return {e.__name__: make(e) for e in edits if names is None or e.__name__ in names}


class _ModesGeometry:
    """synth.Geometry in the shape tests/enc_modes_ref.dc_residuals reads."""

    def __init__(self, geom):
        self.nfrags = geom.nfrags
        self.planes = [dict(nhfrags=geom.nh[p], nvfrags=geom.nv[p], froffset=geom.froffset[p], nfrags=geom.pl_nfrags[p]) for p in range(3)]


def predicted_residuals(geom, frame):
    """The DC residual of every coded fragment (coded order) when the frame's DC values are predicted as section 7.8 says
    (tests/enc_modes_ref.dc_residuals): what the tokens at index 0 carry when `dc` is NULL."""
    from tests import enc_modes_ref
    cf = np.asarray(frame["coded_fragis"], np.int64)
    lev = np.zeros((geom.nfrags, 1), np.int64)
    lev[cf, 0] = np.asarray(frame["coeffs"], np.int64).reshape(-1, 64)[:, 0]
    coded = np.zeros(geom.nfrags, bool)
    coded[cf] = True
    cls = (np.asarray(frame["refi"], np.int64) + 1).tolist()   # a class per reference frame
    dcr = enc_modes_ref.dc_residuals(_ModesGeometry(geom), lev, coded.tolist(), cls, 3)
    out = dcr[cf]
    assert (np.abs(out) < 32768).all()
    return out.astype(np.int16)
