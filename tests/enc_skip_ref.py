"""enc_skip_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s skip decision (TH_ENCCTL_THIP_SET_RD_SKIP;
include/theoraenc_hip.h, "Skip decision") in numpy and plain loops, to compare the library's blocks and packets with byte for byte.
Integer arithmetic throughout (Python ints in the test itself).

The searches and mode rules are the restated encoders' (tests/enc_inter_ref.py, enc_modes_ref.py, enc_rd_ref.py), the block-qi choice
and masking's scales tests/enc_bqi_ref.py's and tests/enc_mask_ref.py's, the transform and the quantiser the oracle's.  What is new:
the test per block, luma before chroma, and the chroma of a macro block that lost its mode.  SkipEncoder is enc_rd_ref.RdEncoder with
the rule behind its block coding; with the switch off it is RdEncoder.
"""
import numpy as np

import oracle
from tests import enc_bqi_ref as B
from tests import enc_inter_ref as IR
from tests import enc_mask_ref as K
from tests import enc_modes_ref as M
from tests import enc_rd_ref as R
from tests import enc_ref
from tests.enc_inter_ref import mode_bits, mv_vlc_bits, predict
from tests.enc_modes_ref import GOLDEN_MV, GOLDEN_NOMV, INTRA, MV, MV_FOUR, MV_LAST, MV_LAST2, NOMV
from tests.enc_ref import ZIGZAG
from tests.streamgen import MODE_ALPHABETS, MODE_REFI, BitWriter, write_long_runs, write_mv, write_short_runs

SSD_SHIFT = 4    # D_skip = SSD << 4 ...
MV_DOUBLE = 2    # ... times this when the block's vector is not (0, 0)


def block_lambda(tab0, iscale=None, lam_fix=None):
    """lambda_b of a block whose table at qis[0] is tab0 (zig-zag): block qi's lambda, or lam_fix in its place (the stage's `lambda`),
    scaled by masking's iscale (Q11) where there is one."""
    s = int(tab0[1])
    lam = (s * s * B.LAM_NUM) >> B.LAM_SHIFT if lam_fix is None else int(lam_fix)
    return lam if iscale is None else (lam * int(iscale) + 1024) >> 11


def code_block(c, tabs, bits, lam_b, bias=B.FLAG_BIAS):
    """One block: c [64] its fDCT (zig-zag), tabs the block's table at each qi of the list, bits [4][32] of its plane, lam_b its
    lambda.  Returns (levels with the DC at qis[0] and the AC at the chosen qi, qii, D_code, R)."""
    c = [int(v) for v in c]
    cand = block_candidates(c, tabs, bits)
    k = choose_candidate(cand, lam_b, bias)
    q, d, r = cand[k]
    lev = cand[0][0].copy()
    lev[1:] = q[1:]
    d_code = d + (c[0] - int(lev[0]) * int(tabs[0][0])) ** 2
    return lev, k, d_code, r


def block_candidates(c, tabs, bits):
    """The block's candidates, one a qi of the list: [(levels [64] int64, D_k: the squared error at z >= 1, R_k: the AC bits)], on
    Python ints.  A level beyond +-580 counts as token 22 does, whose length does not depend on the value."""
    c = [int(v) for v in c]
    cand = []
    for tab in tabs:
        q = oracle.quantize_batch(np.asarray([c], np.int16), np.asarray(tab, np.uint16))[0][0].astype(np.int64)
        d = sum((c[z] - int(q[z]) * int(tab[z])) ** 2 for z in range(1, 64))
        cand.append((q, d, B.ac_bits(np.clip(q, -580, 580), bits)))
    return cand


def choose_candidate(cand, lam_b, bias=B.FLAG_BIAS):
    """The choice rule: the least D_k + lam_b (R_k + bias for k != 0), a tie to the lower k."""
    return min((d + int(lam_b) * (r + (bias if k else 0)), k) for k, (_, d, r) in enumerate(cand))[1]


def skip_test(ssd, moving, d_code, lam_b, r):
    """(D_skip, whether the block is left uncoded)."""
    d_skip = (int(ssd) << SSD_SHIFT) * (MV_DOUBLE if moving else 1)
    return d_skip, d_skip <= int(d_code) + int(lam_b) * int(r)


def skip_code(geo, src, prev, gold, pix, mv, bmv, tabs, bits2, iscale=None, lam_fix=None, bias=B.FLAG_BIAS):
    """The frame's blocks under the rule.  src, prev, gold: three planes each, bitstream rows (gold may be None without GOLD modes);
    pix [nmbs], mv [nmbs, 2], bmv [nmbs, 4, 2]: the macro blocks' decisions; tabs: a list over the qi list of {(qti, plane): zig-zag
    steps}; bits2: (luma, chroma) [4][32]; iscale: [nfrags] or None; lam_fix: None, or the unscaled lambda of every block.
    Returns a dict of raster-order arrays: lev [nfrags, 64], qii, qti, cls, coded, skf, dcode, rate, dskip, fvx, fvy (zero where a
    macro block lost its mode), and demoted [nmbs]."""
    pix, mv = np.asarray(pix, np.int64), np.asarray(mv, np.int64)
    bmv = np.zeros((len(pix), 4, 2), np.int64) if bmv is None else np.asarray(bmv, np.int64)
    fvx, fvy = M.fragment_vectors(geo, pix, mv, bmv)
    fvx, fvy = fvx.copy(), fvy.copy()
    fpix = pix[geo.mb_of].copy()
    nf = geo.nfrags
    out = dict(lev=np.zeros((nf, 64), np.int64), qii=np.zeros(nf, np.int64), qti=np.ones(nf, np.int64), cls=np.zeros(nf, np.int64),
               coded=np.zeros(nf, bool), skf=np.zeros(nf, bool), dcode=np.zeros(nf, np.int64), rate=np.zeros(nf, np.int64),
               dskip=np.zeros(nf, np.int64))
    r8 = np.arange(8)

    def plane(p):
        g = geo.planes[p]
        nh, o = g["nhfrags"], g["froffset"]
        qx, qy = p > 0 and geo.hdec, p > 0 and geo.vdec
        for loc in range(g["nfrags"]):
            f = o + loc
            Y, X = (loc // nh) * 8 + r8[:, None], (loc % nh) * 8 + r8[None, :]
            s = src[p][Y, X].astype(np.int64)
            m = int(fpix[f])
            if m == INTRA:
                pred = 128
            else:
                ref = gold if m in (GOLDEN_NOMV, GOLDEN_MV) else prev
                pred = predict(ref[p], X, Y, int(fvx[f]), int(fvy[f]), qx, qy)
            qti = 0 if m == INTRA else 1
            c = oracle.fdct8x8_batch((s - pred).reshape(1, 64).astype(np.int16))[0]
            tb = [t[(qti, p)] for t in tabs]
            lam_b = block_lambda(tb[0], None if iscale is None else iscale[f], lam_fix)
            lev, k, d_code, r = code_block(c, tb, bits2[int(p > 0)], lam_b, bias)
            ssd = int(((s - prev[p][Y, X].astype(np.int64)) ** 2).sum())
            d_skip, skip = skip_test(ssd, fvx[f] != 0 or fvy[f] != 0, d_code, lam_b, r)
            wanted = m != NOMV or bool(lev.any())
            skipped = wanted and not (m == MV_FOUR and p == 0) and skip
            out["lev"][f], out["qii"][f], out["qti"][f] = lev, k, qti
            out["cls"][f] = 1 if qti == 0 else 3 if m in (GOLDEN_NOMV, GOLDEN_MV) else 2
            out["coded"][f], out["skf"][f] = wanted and not skipped, skipped
            out["dcode"][f], out["rate"][f], out["dskip"][f] = d_code, r, d_skip

    plane(0)
    nh0 = geo.planes[0]["nhfrags"]
    demoted = np.zeros(len(pix), bool)
    for mb in range(len(pix)):
        f0 = 2 * (mb // geo.nmbx) * nh0 + 2 * (mb % geo.nmbx)
        demoted[mb] = not out["coded"][[f0, f0 + 1, f0 + nh0, f0 + nh0 + 1]].any()
    lost = demoted[geo.mb_of]   # to the decoder these macro blocks are INTER_NOMV
    fpix[lost], fvx[lost], fvy[lost] = NOMV, 0, 0
    plane(1)
    plane(2)
    # a macro block "lost its mode" when the test took its last coded luma block (not when the rules before it left none)
    skl = out["skf"][:geo.planes[0]["nfrags"]]
    took = np.zeros(len(pix), bool)
    np.logical_or.at(took, geo.mb_of[:len(skl)], skl)
    return dict(out, fvx=fvx, fvy=fvy, fpix=fpix, demoted=demoted & took)


def stage_bits(setup, hti):
    """uint8 [2][4][32] as thip_enc_skip_stage takes it: luma then chroma, code length + extra bits of every token in the AC Huffman
    groups 1..4 of tables hti[0], hti[1]."""
    from tests.packref import EXTRA_BITS
    return (np.asarray([B.token_bits(setup, t) for t in hti], np.int64) + np.asarray(EXTRA_BITS, np.int64)[None, None, :]).astype(np.uint8)


def stage(geo, src, prev, gold, pix, mv, bmv, dequant, bits, iscale=None, lam_fix=None):
    """skip_code in thip_enc_skip_stage's shapes: dequant [nqis][2][3][64], bits uint8 [2][4][32].  dict(levels [nfrags, 64] int16 and
    qii, dcode, rate, dskip in CODED order; dcq, cmap, skf raster)."""
    dq = np.asarray(dequant, np.int64).reshape(-1, 2, 3, 64)
    tabs = [{(t, p): dq[k, t, p] for t in range(2) for p in range(3)} for k in range(dq.shape[0])]
    from tests.packref import EXTRA_BITS
    # (the entry's table holds code length + extra bits; enc_bqi_ref.ac_bits adds a token's extra bits itself)
    b = (np.asarray(bits, np.int64).reshape(2, 4, 32) - np.asarray(EXTRA_BITS, np.int64)[None, None, :]).tolist()
    d = skip_code(geo, src, prev, gold, pix, mv, bmv, tabs, b, iscale, lam_fix)
    co = geo.coded_order
    return dict(levels=d["lev"][co].astype(np.int16), qii=d["qii"][co].astype(np.uint8), dcode=d["dcode"][co], rate=d["rate"][co],
                dskip=d["dskip"][co], dcq=d["lev"][:, 0].astype(np.int16), cmap=(d["coded"] * d["cls"]).astype(np.uint8),
                skf=d["skf"].astype(np.uint8), demoted=d["demoted"])


# ---- the stream ----------------------------------------------------------------------------------------------------------------
class _SkipInter(K.MaskEncoder):
    """MaskEncoder whose inter frames run the rule behind the block coding (BqiEncoder._inter with skip_code in place of _code and of
    the coded rule); enc_rd_ref.RdEncoder in front of it hands it the rate-distortion decision as it hands it to BqiEncoder."""
    skip = True

    def _inter(self, planes, qi):
        if not self.skip:
            return super()._inter(planes, qi)
        geo, setup = self.geo, self.setup
        qis = B.qi_list(qi, self.delta)
        src = [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]
        prev = [self.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)]
        gold = [self.ost.get_plane(oracle.FRAME_GOLD, p) for p in range(3)]
        s1 = int(setup.qmat(1, 0, qi)[ZIGZAG][1])
        if self.modes:
            ms = M.motion_search(src[0], prev[0], gold[0], s1)
            pix, mv, bmv = ms["pix"], ms["mv"], ms["bmv"]
        else:
            pix, mvx, mvy = IR.motion_search(src[0], prev[0], s1)[:3]
            mv = np.stack([mvx, mvy], 1)
            bmv = np.zeros((len(pix), 4, 2), np.int64)
        iscale = None
        if self.k and self.delta:
            iscale, A, amax = K.scales(K.activity(self._planes, self.fw, self.fh, self.fmt, self.pic), self.k, geo)
            self._mask = (A, amax)
        tabs = [{(t, p): setup.qmat(t, p, q)[ZIGZAG] for t in range(2) for p in range(3)} for q in qis]
        ht = self.hti[False]
        d = skip_code(geo, src, prev, gold, pix, mv, bmv, tabs, [B.token_bits(setup, ht[0]), B.token_bits(setup, ht[1])], iscale,
                      bias=self.bias)
        lev, qii, qti_of, cls, coded, fvx, fvy = d["lev"], d["qii"], d["qti"], d["cls"], d["coded"], d["fvx"], d["fvy"]
        if not coded.any():
            return dict(packet=b"", modes=[0] * 5, coded=[0, 0, 0], mode_scheme=-1, mv_scheme=-1)
        self._skip = dict(skipped=[int(d["skf"][geo.froff[p]:geo.froff[p] + g["nfrags"]].sum()) for p, g in enumerate(geo.planes)],
                          demoted=int(d["demoted"].sum()), lam=(s1 * s1 * B.LAM_NUM) >> B.LAM_SHIFT, detail=d)
        bw = BitWriter()
        self._header(bw, False, qis)
        # 7.3 coded flags
        sbp, sbf, blk, at = [], [], [], 0
        for n in geo.sb_len:
            c = coded[geo.coded_order[at:at + n]]
            partial = 0 < c.sum() < n
            sbp.append(int(partial))
            if partial:
                blk.extend(int(v) for v in c)
            else:
                sbf.append(int(c.all()))
            at += n
        write_long_runs(bw, sbp)
        write_long_runs(bw, sbf)
        write_short_runs(bw, blk)
        # 7.4 modes, 7.5 vectors: a macro block with no coded luma block writes neither
        nh0 = geo.planes[0]["nhfrags"]
        modes, mvs, last1, last2 = [], [], (0, 0), (0, 0)
        counts = [0] * 8
        mb_mode = np.full(len(pix), NOMV)
        for mb in geo.mb_order:
            f0 = 2 * (mb // geo.nmbx) * nh0 + 2 * (mb % geo.nmbx)
            if not (coded[f0] or coded[f0 + 1] or coded[f0 + nh0] or coded[f0 + nh0 + 1]):
                counts[NOMV] += 1
                continue
            mode = int(pix[mb])
            if mode == MV:
                v = (int(mv[mb, 0]), int(mv[mb, 1]))
                if v == last1:
                    mode = MV_LAST
                elif v == last2:
                    mode = MV_LAST2
                    last2, last1 = last1, v
                else:
                    mvs.append(v)
                    last2, last1 = last1, v
            elif mode == MV_FOUR:
                for k in range(4):
                    mvs.append((int(bmv[mb, k, 0]), int(bmv[mb, k, 1])))
                last2, last1 = last1, mvs[-1]
            elif mode == GOLDEN_MV:
                mvs.append((int(mv[mb, 0]), int(mv[mb, 1])))
            modes.append(mode)
            mb_mode[mb] = mode
            counts[mode] += 1
        freq = [modes.count(m) for m in range(8)]
        alpha0 = sorted(range(8), key=lambda m: -freq[m])
        rank0 = [alpha0.index(m) for m in range(8)]
        scheme = int(np.argmin([mode_bits(freq, s, rank0) for s in range(8)]))
        bw.write(scheme, 3)
        if scheme == 0:
            for m in range(8):
                bw.write(rank0[m], 3)
        for m in modes:
            if scheme == 7:
                bw.write(m, 3)
            else:
                i = rank0[m] if scheme == 0 else MODE_ALPHABETS[scheme - 1].index(m)
                bw.code("1" * i + ("0" if i < 7 else ""))
        vlc = sum(mv_vlc_bits(c) for v in mvs for c in v)
        mvmode = 1 if vlc > 6 * 2 * len(mvs) else 0
        bw.write(mvmode, 1)
        for v in mvs:
            write_mv(bw, v[0], mvmode)
            write_mv(bw, v[1], mvmode)
        ost = self.ost
        ost.coded[:] = coded
        refi = np.array([MODE_REFI[int(m)] for m in mb_mode[geo.mb_of]], np.uint8)
        refi[~coded] = 3
        ost.refi[:] = refi
        ost.mvs[:] = ((fvx & 0xFF) | (fvy << 8)).astype(np.int16)
        out = self._finish(bw, lev, qii, qti_of, coded, cls, qis, False, qi)
        out.update(modes=counts[:5], modes8=counts, vectors=len(mvs), mode_scheme=scheme, mv_scheme=mvmode, pix=pix)
        return out


class SkipEncoder(R.RdEncoder, _SkipInter):
    """The stream th_encode_* makes with TH_ENCCTL_THIP_SET_RD_SKIP on (skip=False: off, RdEncoder's stream), five or eight modes,
    block qi `delta`, masking `k`, the rate-distortion mode decision `rd` (eight modes only).  frame() returns RdEncoder's dict plus
    skip (TH_ENCCTL_THIP_GET_SKIP_STATS as Encoder.skip_stats returns it, without skip_ms) and, for a frame decided by the rule,
    skip_detail (skip_code's dict)."""

    def __init__(self, fw, fh, fmt, pic, setup, kf_interval, shift, delta=0, k=0, modes=True, rd=False, skip=True):
        super().__init__(fw, fh, fmt, pic, setup, kf_interval, shift, delta, k, modes, rd and modes)
        self.skip = skip
        self._skip = None

    def frame(self, planes, qi, dups=0):
        self._skip = None
        self._planes = planes
        out = super().frame(planes, qi, dups)
        m = self._skip if out["packet"] else None
        out["skip"] = dict(on=int(self.skip), measured=int(m is not None), skipped=m["skipped"] if m else [0] * 3,
                           demoted=m["demoted"] if m else 0, lam=m["lam"] if m else 0)
        if m:
            out["skip_detail"] = m["detail"]
        return out


class CutSkipEncoder(SkipEncoder, R.enc_cut_ref.CutBase):
    """SkipEncoder with automatic key frames at ratio self.t."""


class RateStream(R.enc_rate_ref.RateStream):
    """enc_rate_ref's bitrate-mode stream with SkipEncoder: the probe and the controller are unchanged."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, fps=(30, 1), kf_interval=64, shift=6, delta=0, k=0, modes=True, rd=False, **kw):
        super().__init__(fw, fh, fmt, pic, setup, bitrate, fps=fps, inter=True, kf_interval=kf_interval, shift=shift, **kw)
        self.enc.close()
        self.enc = SkipEncoder(fw, fh, fmt, pic, setup, kf_interval, shift, delta, k, modes, rd)


# ---- content ------------------------------------------------------------------------------------------------------------------
def clip(kind, fw, fh, fmt, nframes, seed=0):
    """Frames (three top-first planes each) of frame size fw x fh:
      static  a still, textured background; a small textured object (a sixth of the frame a side) moves across it three luma pixels a
              frame, and every frame carries a little noise of its own (one grey level on one pixel in four): the content the rule
              exists for -- most blocks change by less than coding them would mend
      pan     enc_inter_ref.sequence's pan"""
    if kind != "static":
        return IR.sequence(kind, fw, fh, fmt, nframes, seed)
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    bg = [enc_ref.content("natural", (fh, fw), seed + p) for p in range(3)]
    ob = [enc_ref.content("natural", (fh, fw), seed + 17 + p) for p in range(3)]
    rng = np.random.default_rng(seed + 5)
    oh, ow = max(fh // 6, 8) & ~1, max(fw // 6, 8) & ~1
    out = []
    for f in range(nframes):
        ox, oy = (4 + 3 * f) % max(fw - ow, 1) & ~1, (fh // 3) & ~1
        fr = []
        for p in range(3):
            sx, sy = (hd, vd) if p else (0, 0)
            a = bg[p][::1 + sy, ::1 + sx].astype(np.int64)
            a[oy >> sy:(oy + oh) >> sy, ox >> sx:(ox + ow) >> sx] = ob[p][:((oy + oh) >> sy) - (oy >> sy), :((ox + ow) >> sx) - (ox >> sx)]
            noise = (rng.integers(0, 4, a.shape) == 0) * rng.integers(-1, 2, a.shape)
            fr.append(np.ascontiguousarray(np.clip(a + noise, 0, 255).astype(np.uint8)))
        out.append(fr)
    return out


# ---- the packet cases of tests/test_gpu_encoder_skip.py (tests/test_encoder_skip_cpu.py asserts that they are not vacuous) ---------
# (clip kind, frame width, height, pixel format, quality, frames, modes, block qi, masking, rd)
PACKET_CASES = [("static", 64, 48, 0, 32, 3, False, 0, 0, False), ("static", 64, 48, 2, 16, 3, True, 0, 0, False),
                ("static", 64, 48, 3, 48, 3, True, 8, 4, False), ("pan", 64, 48, 0, 12, 3, True, 0, 0, True),
                ("pan", 64, 48, 3, 16, 3, False, 8, 0, False), ("static", 176, 144, 0, 32, 3, True, 8, 4, True),
                ("pan", 176, 144, 0, 8, 3, True, 0, 0, False)]


def case_frames(case):
    return clip(case[0], case[1], case[2], case[3], case[5], seed=case[4])


def case_encoder(case, setup, skip=True):
    kind, w, h, fmt, q, nf, modes, delta, k, rd = case
    return SkipEncoder(w, h, fmt, (0, 0, w, h), setup, 64, 6, delta, k, modes, rd, skip)
