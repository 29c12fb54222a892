"""th_encode_* without a GPU: th_info validation, th_encode_ctl, the three headers (read back by the library's own decoder and by
tests/enc_ref.py's parser), granule arithmetic on an encoder context.  Nothing here reaches the first th_encode_ycbcr_in, which is
where the encoder first touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import enc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from theora_amd import _lib as L
    return L, L.load()


def test_encoder_header_and_exports_agree():
    """include/theoraenc_hip.h <-> ENC_SYMBOLS <-> exported symbols; theoradec_hip.h declares none of them."""
    from theora_amd import _lib as Lm
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "theoraenc_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(th_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(n for n, _, _ in Lm.ENC_SYMBOLS)
    dec = open(os.path.join(ROOT, "include", "theoradec_hip.h")).read()
    assert "th_encode" not in re.sub(r"/\*.*?\*/", "", dec, flags=re.S)
    L = Lm.load()
    for name in declared:
        assert hasattr(L, name), name


def _alloc(L, **kw):
    from theora_amd.encoder import make_info
    args = dict(w=64, h=48, fmt=0, quality=32)
    args.update({k: kw.pop(k) for k in list(kw) if k in ("w", "h", "fmt", "quality")})
    info = make_info(args["w"], args["h"], args["fmt"], args["quality"])
    for k, v in kw.items():
        setattr(info, k, v)
    return L.th_encode_alloc(C.byref(info)), info


@pytest.mark.parametrize("field", [
    dict(w=0), dict(h=0), dict(w=40), dict(h=56 + 4), dict(fmt=1), dict(fmt=4), dict(quality=-1), dict(quality=64),
    dict(keyframe_granule_shift=-1), dict(keyframe_granule_shift=32), dict(target_bitrate=100000),
    dict(pic_width=65), dict(pic_height=49), dict(pic_x=1), dict(pic_y=1), dict(pic_width=0),
])
def test_alloc_rejects_invalid_info(field):
    _, L = _lib()
    enc, _ = _alloc(L, **field)
    assert not enc


def test_alloc_accepts_valid_info():
    _, L = _lib()
    for fmt in (0, 2, 3):
        enc, _ = _alloc(L, fmt=fmt, pic_x=1, pic_y=2, pic_width=61, pic_height=45)
        assert enc
        L.th_encode_free(enc)


def test_ctl_values():
    from theora_amd import encoder as E
    Lm, L = _lib()
    enc, _ = _alloc(L)
    try:
        def ctl(req, val, ctype=C.c_int, size=None):
            v = ctype(val)
            return L.th_encode_ctl(enc, req, C.byref(v), C.sizeof(v) if size is None else size), v.value
        assert ctl(E.TH_ENCCTL_SET_QUALITY, 40) == (0, 40)
        assert ctl(E.TH_ENCCTL_SET_QUALITY, 64)[0] == Lm.EINVAL
        assert ctl(E.TH_ENCCTL_SET_KEYFRAME_FREQUENCY_FORCE, 64, C.c_uint32) == (0, 1)
        assert ctl(E.TH_ENCCTL_SET_DUP_COUNT, 3) == (0, 3)
        assert ctl(E.TH_ENCCTL_GET_SPLEVEL_MAX, 7) == (0, 0)
        assert ctl(E.TH_ENCCTL_SET_SPLEVEL, 0)[0] == 0
        assert ctl(E.TH_ENCCTL_SET_SPLEVEL, 1)[0] == Lm.EINVAL
        for req in (0, 2, 10, 16, 20, 22, 24, 26, 30, 32, 0x7299):
            assert ctl(req, 0)[0] == Lm.EIMPL, req
        assert ctl(E.TH_ENCCTL_SET_QUALITY, 40, size=8)[0] == Lm.EINVAL
        assert L.th_encode_ctl(None, E.TH_ENCCTL_SET_QUALITY, None, 0) == Lm.EFAULT
    finally:
        L.th_encode_free(enc)


def _headers(w=64, h=48, fmt=0, quality=32, pic=None, fps=(30, 1), kfgshift=6, comments=()):
    from theora_amd.encoder import Encoder
    e = Encoder(w, h, fmt, quality, pic=pic, fps=fps, kfgshift=kfgshift, comments=comments)
    hdr = e.header_packets()
    return e, hdr


def test_flushheader_returns_three_then_zero():
    from theora_amd import _lib as Lm
    e, hdr = _headers()
    assert len(hdr) == 3 and [p[0] for p in hdr] == [0x80, 0x81, 0x82]
    op, tc = Lm.OggPacket(), Lm.ThComment()
    e._L.th_comment_init(C.byref(tc))
    assert e._L.th_encode_flushheader(e._enc, C.byref(tc), C.byref(op)) == 0
    assert e._L.th_encode_flushheader(e._enc, None, C.byref(op)) == Lm.EFAULT
    e.close()


@pytest.mark.parametrize("w,h,fmt,pic,fps,shift", [
    (64, 48, 0, (1, 2, 61, 45), (30000, 1001), 6), (176, 144, 2, None, (25, 1), 0), (32, 32, 3, (0, 5, 31, 27), (24, 1), 31),
])
def test_headers_round_trip_through_decoder(w, h, fmt, pic, fps, shift):
    e, hdr = _headers(w, h, fmt, 20, pic=pic, fps=fps, kfgshift=shift, comments=["TITLE=enc", "ARTIST=hip encoder"])
    try:
        from theora_amd import _lib as Lm
        L = Lm.load()
        info, tc = Lm.ThInfo(), Lm.ThComment()
        L.th_info_init(C.byref(info))
        L.th_comment_init(C.byref(tc))
        setup = C.c_void_p()
        for k, pkt in enumerate(hdr):
            buf = (C.c_ubyte * len(pkt)).from_buffer_copy(pkt)
            op = Lm.OggPacket(C.cast(buf, C.c_void_p), len(pkt), int(k == 0), 0, 0, k)
            assert L.th_decode_headerin(C.byref(info), C.byref(tc), C.byref(setup), C.byref(op)) > 0
        x, y, pw, ph = pic if pic else (0, 0, w, h)
        got = {f: getattr(info, f) for f, _ in Lm.ThInfo._fields_}
        want = {f: getattr(e.info, f) for f, _ in Lm.ThInfo._fields_}
        want.update(version_major=3, version_minor=2, version_subminor=1)
        assert got == want
        assert (info.pic_x, info.pic_y, info.pic_width, info.pic_height) == (x, y, pw, ph)
        assert (info.fps_numerator, info.fps_denominator, info.keyframe_granule_shift, info.pixel_fmt) == (*fps, shift, fmt)
        assert C.string_at(tc.vendor) == L.th_version_string()
        assert [C.string_at(tc.user_comments[k], tc.comment_lengths[k]) for k in range(tc.comments)] == \
            [b"TITLE=enc", b"ARTIST=hip encoder"]
        L.th_setup_free(setup)
        L.th_comment_clear(C.byref(tc))
    finally:
        e.close()


def test_setup_header_trees_and_quantisers():
    """80 complete prefix codes over all 32 tokens, none longer than 32 bits; every quantiser step non-increasing in qi; the
    parser consumes the whole header."""
    e, hdr = _headers()
    s = enc_ref.SetupParams(hdr[2])
    assert s.bits_used <= len(hdr[2]) * 8 < s.bits_used + 8
    for codes in s.codes:
        assert sorted(codes) == list(range(32))
        assert max(len(c) for c in codes.values()) <= 32
        assert abs(sum(2.0 ** -len(c) for c in codes.values()) - 1.0) < 1e-12   # complete
        cs = sorted(codes.values())
        assert all(not b.startswith(a) for a, b in zip(cs, cs[1:]))              # prefix-free
    for qti in range(2):
        for pli in range(3):
            q = np.array([s.qmat(qti, pli, qi) for qi in range(64)])
            assert (np.diff(q, axis=0) <= 0).all(), (qti, pli)
            assert q.min() >= (8 if qti == 0 else 16)
    assert all(a >= b for a, b in zip(s.lflims, s.lflims[1:]))
    e.close()


def test_granule_helpers_take_an_encoder_context():
    _, L = _lib()
    for shift in (0, 6):
        enc, _ = _alloc(L, keyframe_granule_shift=shift)
        assert enc
        # 3.2.1 numbering: key frame n (from 0) is (n + 1) << shift, the k-th frame after it adds k
        assert L.th_granule_frame(enc, (5 << shift) + (2 if shift else 0)) == 4 + (2 if shift else 0)
        assert L.th_granule_frame(enc, 1 << shift) == 0
        assert abs(L.th_granule_time(enc, 1 << shift) - 1 / 30) < 1e-12
        assert L.th_granule_frame(enc, -1) == -1
        L.th_encode_free(enc)


def test_packetout_before_any_frame_and_bad_buffers():
    from theora_amd import _lib as Lm
    e, _ = _headers()
    op = Lm.OggPacket()
    assert e._L.th_encode_packetout(e._enc, 0, C.byref(op)) == 0
    assert e._L.th_encode_packetout(e._enc, 1, C.byref(op)) == 0
    buf = (Lm.ThImgPlane * 3)()
    data = (C.c_ubyte * 64)()
    for p in range(3):   # neither frame nor picture size: refused before anything reaches the device
        buf[p].width, buf[p].height, buf[p].stride = 8, 8, 8
        buf[p].data = C.cast(data, C.POINTER(C.c_ubyte))
    assert e._L.th_encode_ycbcr_in(e._enc, buf) == Lm.EINVAL
    assert e._L.th_encode_ycbcr_in(e._enc, None) == Lm.EFAULT
    e.close()


def _crc_ok(page):
    """RFC 3533 CRC of one page (polynomial 0x04c11db7, direct, initial 0), the checksum field taken as zero."""
    crc = 0
    data = page[:22] + b"\0\0\0\0" + page[26:]
    for byte in data:
        crc ^= byte << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc == int.from_bytes(page[22:26], "little")


def _pages(data):
    out, pos = [], 0
    while pos < len(data):
        assert data[pos:pos + 4] == b"OggS" and data[pos + 4] == 0
        nseg = data[pos + 26]
        size = 27 + nseg + sum(data[pos + 27:pos + 27 + nseg])
        out.append(data[pos:pos + size])
        pos += size
    return out


def test_ogg_writer_round_trip_through_the_reader():
    """thip_ogg_writer -> thip_ogg_reader: packets (empty ones, 255-byte multiples, packets over several pages), granule
    positions, BOS / EOS, valid CRCs, the page rule of include/thip_ogg.h."""
    from theora_amd.decoder import ogg_packets
    from theora_amd.encoder import ogg_stream
    rng = np.random.default_rng(4)
    hdr = [b"\x80theora" + bytes(35), b"\x81theora" + bytes(300), b"\x82theora" + rng.integers(0, 256, 3000, np.uint8).tobytes()]
    sizes = [0, 1, 254, 255, 510, 70000, 4095, 4096, 0, 17, 255 * 255, 300]
    data = [(rng.integers(0, 256, n, np.uint8).tobytes(), (k + 1) << 6, int(k == len(sizes) - 1)) for k, n in enumerate(sizes)]
    ogv = ogg_stream(hdr, data, serialno=0xC0FFEE)
    pages = _pages(ogv)
    assert all(_crc_ok(p) for p in pages)
    assert [p[5] & 2 for p in pages] == [2] + [0] * (len(pages) - 1)                 # BOS on the first page only
    assert [p[5] & 4 for p in pages] == [0] * (len(pages) - 1) + [4]                 # EOS on the last
    assert pages[0][26] == 1 and pages[0][27] == len(hdr[0])                          # the first header alone on its page
    assert int.from_bytes(pages[0][14:18], "little") == 0xC0FFEE
    assert [int.from_bytes(p[18:22], "little") for p in pages] == list(range(len(pages)))
    # the setup header ends a page: the header pages (granule 0) hold the headers and nothing else
    gran = [int.from_bytes(p[6:14], "little", signed=True) for p in pages]
    body = [len(p) - 27 - p[26] for p in pages]
    assert sum(b for b, g in zip(body, gran) if g == 0) == sum(len(x) for x in hdr)
    assert gran[:2] == [0, 0] and 0 not in gran[2:]
    got, (bad, gaps) = ogg_packets(ogv)
    assert (bad, gaps) == (0, 0)
    assert [g[1] for g in got] == hdr + [d[0] for d in data]
    assert all(g[0] == 0xC0FFEE for g in got)
    assert got[0][2] == 1 and got[-1][3] == 1
    # the granule of a page is that of its last finished packet: every data packet that ends a page reports its own
    for (payload, gp, eos), g in zip(data, got[3:]):
        assert g[4] in (-1, gp)
    assert got[-1][4] == data[-1][1]


def test_ogg_writer_refuses_bad_sequences():
    from theora_amd import _lib as Lm
    L = Lm.load()
    w = L.thip_ogg_writer_new(1)
    buf = (C.c_ubyte * 4)()
    op = Lm.OggPacket(C.cast(buf, C.c_void_p), 4, 0, 0, 0, 0)
    assert L.thip_ogg_writer_packetin(w, C.byref(op)) == -1          # the first packet must open the stream
    op.b_o_s, op.e_o_s = 1, 1
    assert L.thip_ogg_writer_packetin(w, C.byref(op)) == 0
    op.b_o_s, op.e_o_s = 0, 0
    assert L.thip_ogg_writer_packetin(w, C.byref(op)) == -1          # nothing after e_o_s
    L.thip_ogg_writer_free(w)


def test_dup_count_limit_follows_the_granule_shift():
    from theora_amd import encoder as E
    Lm, L = _lib()
    for shift, ok, bad in ((6, 63, 64), (1, 1, 2), (0, 1000, None)):
        enc, _ = _alloc(L, keyframe_granule_shift=shift)
        v = C.c_int(ok)
        assert L.th_encode_ctl(enc, E.TH_ENCCTL_SET_DUP_COUNT, C.byref(v), C.sizeof(v)) == 0
        if bad is not None:
            v = C.c_int(bad)
            assert L.th_encode_ctl(enc, E.TH_ENCCTL_SET_DUP_COUNT, C.byref(v), C.sizeof(v)) == Lm.EINVAL
        L.th_encode_free(enc)
