"""numpy restatement of thip_frame_info_out's definitions (include/theora_hip.h): from what a frame's slot calls say about every
fragment -- coded or not, reference, vector, last_zzi -- to the maps kind / mv / ncoef per plane, the dense luma field flow and
valid, for any rectangle.  Fragments are kept per plane in BITSTREAM order (row 0 at the bottom, as fragment indices run); the
outputs have row 0 at the top."""
import numpy as np

FRAME_GOLD, FRAME_PREV, FRAME_SELF = 0, 1, 2
REF_PREV, REF_GOLD = 1, 2


def decs(pixel_fmt):
    return int(not (pixel_fmt & 1)), int(not (pixel_fmt & 2))


def plane_frags(frame_width, frame_height, pixel_fmt):
    """(nhfrags, nvfrags) per plane (state.c:443-449)."""
    hdec, vdec = decs(pixel_fmt)
    yh, yv = frame_width >> 3, frame_height >> 3
    return [(yh, yv), ((yh + hdec) >> hdec, (yv + vdec) >> vdec), ((yh + hdec) >> hdec, (yv + vdec) >> vdec)]


def empty(frame_width, frame_height, pixel_fmt):
    """Per-fragment arrays of a frame in which nothing is coded: dict of flat arrays over all fragments, fragment-index order."""
    n = sum(nh * nv for nh, nv in plane_frags(frame_width, frame_height, pixel_fmt))
    return dict(coded=np.zeros(n, bool), refi=np.zeros(n, np.int64), mvx=np.zeros(n, np.int64), mvy=np.zeros(n, np.int64),
                last_zzi=np.zeros(n, np.int64))


def from_trace(trace, frame_width, frame_height, pixel_fmt):
    """A slot trace (Decoder.slot_trace(): fragi, refi, mv in OC_MV packing -- x in the low byte, y in the high one, both signed
    --, last_zzi; every fragment not named is on the uncoded list) -> the per-fragment arrays."""
    f = empty(frame_width, frame_height, pixel_fmt)
    fragi = np.asarray(trace["fragi"], np.int64)
    assert np.unique(fragi).size == fragi.size
    unc = np.asarray(trace["uncoded"], np.int64)
    assert fragi.size + unc.size == f["coded"].size and np.intersect1d(fragi, unc).size == 0
    mv = np.asarray(trace["mv"], np.int16).astype(np.int64)
    f["coded"][fragi] = True
    f["refi"][fragi] = np.asarray(trace["refi"], np.int64)
    f["mvx"][fragi] = ((mv & 0xFF) ^ 0x80) - 0x80
    f["mvy"][fragi] = mv >> 8
    f["last_zzi"][fragi] = np.asarray(trace["last_zzi"], np.int64)
    return f


def from_word0(word0):
    """The per-fragment arrays from the word0 of every fragment in fragment-index order (include/theora_hip.h, frag_info)."""
    w = np.asarray(word0, np.uint32).astype(np.int64)
    return dict(coded=(w & 1) != 0, refi=(w >> 1) & 3, mvx=(((w >> 16) & 0xFF) ^ 0x80) - 0x80, mvy=(((w >> 24) & 0xFF) ^ 0x80) - 0x80,
                last_zzi=(w >> 8) & 127)


def frag_rect(rect, p, pixel_fmt):
    """(first column, first row from the top, columns, rows) of the fragments of plane p that the pixel rectangle touches."""
    x, y, w, h = rect
    hdec, vdec = decs(pixel_fmt) if p else (0, 0)
    c0, r0 = (x >> hdec) >> 3, (y >> vdec) >> 3
    return c0, r0, (((x + w - 1) >> hdec) >> 3) - c0 + 1, (((y + h - 1) >> vdec) >> 3) - r0 + 1


def plane_maps(f, frame_width, frame_height, pixel_fmt):
    """Per plane, the whole plane's (kind, vx, vy, ncoef) as 2-D arrays with row 0 at the TOP."""
    out, off = [], 0
    for nh, nv in plane_frags(frame_width, frame_height, pixel_fmt):
        sl = slice(off, off + nh * nv)
        off += nh * nv
        coded, refi = f["coded"][sl], f["refi"][sl]
        kind = np.where(~coded, 0, np.where(refi == FRAME_SELF, 1, np.where(refi == FRAME_PREV, 2, 3)))
        has = kind >= 2
        vx = np.where(has, f["mvx"][sl], 0)
        vy = np.where(has, -f["mvy"][sl], 0)
        vy = ((vy + 128) & 255) - 128           # (the negation is an int8's)
        ncoef = np.where(coded, f["last_zzi"][sl], 0)
        out.append(tuple(a.reshape(nv, nh)[::-1] for a in (kind, vx, vy, ncoef)))   # bottom-up -> top-down
    return out


def frame_info(f, frame_width, frame_height, pixel_fmt, rect=None, refs=REF_PREV, dtype=np.float16):
    """Every output of thip_frame_info_out for the rectangle (None: the whole frame): dict(kind, mv, ncoef: lists of three;
    flow; valid)."""
    if rect is None:
        rect = (0, 0, frame_width, frame_height)
    x, y, w, h = rect
    assert x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= frame_width and y + h <= frame_height
    maps = plane_maps(f, frame_width, frame_height, pixel_fmt)
    res = dict(kind=[], mv=[], ncoef=[])
    for p, (kind, vx, vy, ncoef) in enumerate(maps):
        c0, r0, fw, fh = frag_rect(rect, p, pixel_fmt)
        s = (slice(r0, r0 + fh), slice(c0, c0 + fw))
        res["kind"].append(kind[s].astype(np.uint8))
        res["mv"].append(np.stack([vx[s], vy[s]], axis=-1).astype(np.int8))
        res["ncoef"].append(ncoef[s].astype(np.uint8))
    kind, vx, vy, _ = maps[0]
    # per pixel: the luma fragment that covers it
    rows = (np.arange(y, y + h) >> 3)[:, None]
    cols = (np.arange(x, x + w) >> 3)[None, :]
    k = kind[rows, cols]
    on = ((k == 2) & bool(refs & REF_PREV)) | ((k == 3) & bool(refs & REF_GOLD))
    res["flow"] = np.stack([np.where(on, vx[rows, cols], 0) / 2.0, np.where(on, vy[rows, cols], 0) / 2.0]).astype(dtype)
    res["valid"] = k.astype(np.uint8)
    return res
