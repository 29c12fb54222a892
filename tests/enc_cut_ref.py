"""enc_cut_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s automatic key frames (TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES;
include/theoraenc_hip.h, "Automatic key frames") in numpy, to compare the library's choices and packets with exactly.

The measurement is tests/enc_rate_ref.py's search_stats (the five-mode search before its decision) summed over the frame; the frames
themselves are the other restatements': enc_inter_ref.InterEncoder (five modes), enc_modes_ref.ModesEncoder (eight), enc_bqi_ref.BqiEncoder
(block qi) and enc_rate_ref.RateStream (bitrate mode).  Each encoder's frame() applies the interval rule, then the measurement, then
codes the frame as its base does.
"""
import numpy as np

import oracle
from tests import enc_bqi_ref, enc_inter_ref, enc_modes_ref, enc_rate_ref, enc_ref

RECOMMENDED = 230          # t: the ratio P / I >= 230 / 256
MIN_ERROR = 4              # P >= MIN_ERROR * 256 * nmbs: a mean absolute prediction error of 4 levels a luma pixel
NO_STATS = dict(measured=0, cut=0, intra_mbs=0, pred=0, intra=0)


def measure(src_luma, ref_luma):
    """(P, I, N) of luma src against ref (both of the frame's size, bitstream row order): P = sum min(S0, Smv), I = sum SI, N = the
    macro blocks with SI < min(S0, Smv)."""
    _, _, _, s0, si, smv = enc_rate_ref.search_stats(src_luma, ref_luma)
    inter = np.minimum(s0, smv)
    return int(inter.sum()), int(si.sum()), int((si < inter).sum())


def decide(P, I, nmbs, t):
    return bool(t) and 256 * P >= t * I and P >= MIN_ERROR * 256 * nmbs


def measure_frame(enc, planes, t):
    """The cut statistics (Encoder.cut_stats's fields, measure_ms apart) of `planes` as the next frame of restated encoder `enc`."""
    src = np.flipud(enc_ref.frame_planes(planes, enc.fw, enc.fh, enc.fmt, enc.pic)[0]).astype(np.int64)
    P, I, N = measure(src, enc.ost.get_plane(oracle.FRAME_PREV, 0))
    return dict(measured=1, cut=int(decide(P, I, len(enc.geo.mb_order), t)), intra_mbs=N, pred=P, intra=I)


class CutBase(enc_inter_ref.InterEncoder):
    """InterEncoder with the switch at ratio self.t: frame() returns the base's dict plus cut (the statistics).  self.forced: a
    (key, statistics) decision made outside (the rate stream's, which decides before its probe), taken once."""
    t = 0
    forced = None

    def frame(self, planes, qi, dups=0):
        f = self.cur + 1
        off = f - self.key
        key = self.key < 0 or off >= self.kf_interval or off + dups >= (1 << self.shift)
        st = dict(NO_STATS)
        if self.forced is not None:
            (key, st), self.forced = self.forced, None
        elif not key and self.t:
            st = measure_frame(self, planes, self.t)
            key = bool(st["cut"])
        out = self._key(planes, qi) if key else self._inter(planes, qi)
        if key:
            self.key = f
        self.cur = f + dups
        out["key"] = key
        out["cut"] = dict(st, ratio=self.t)
        return out


class CutInterEncoder(CutBase):
    pass


class CutModesEncoder(enc_modes_ref.ModesEncoder, CutBase):
    pass


class CutBqiEncoder(enc_bqi_ref.BqiEncoder, CutBase):
    pass


def encoder(t, fw, fh, fmt, pic, setup, kf_interval, shift, modes=False, bqi=0):
    """The restated encoder of those switches with automatic key frames at ratio t (0 off)."""
    if bqi:
        enc = CutBqiEncoder(fw, fh, fmt, pic, setup, kf_interval, shift, bqi, modes=modes)
    else:
        enc = (CutModesEncoder if modes else CutInterEncoder)(fw, fh, fmt, pic, setup, kf_interval, shift)
    enc.t = t
    return enc


class CutRateStream(enc_rate_ref.RateStream):
    """enc_rate_ref's bitrate-mode stream with the switch at ratio t: the decision precedes the probe.  frame(planes, dups) -> list
    of (packet, rate record, cut statistics)."""

    def __init__(self, t, fw, fh, fmt, pic, setup, bitrate, kf_interval=64, shift=6, modes=False, **kw):
        super().__init__(fw, fh, fmt, pic, setup, bitrate, inter=True, kf_interval=kf_interval, shift=shift, **kw)
        self.enc.close()
        self.enc = encoder(t, fw, fh, fmt, pic, setup, kf_interval, shift, modes=modes)
        self.t = t

    def frame(self, planes, dups=0):
        f = self.cur + 1
        off = f - self.key
        key = self.key < 0 or off >= self.K or off + dups >= (1 << self.shift)
        st = dict(NO_STATS)
        if not key and self.t:
            st = measure_frame(self.enc, planes, self.t)
            key = bool(st["cut"])
        if key:
            E = self.probe.key(planes)
        else:
            E = self.probe.inter(planes, [self.enc.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)])
        qi, rec = self.ctl.choose(E, key, f, f if key else self.key, self.cur < 0, self.key, dups)
        rec.update(probe=list(E), key=int(key and qi >= 0))
        out = []
        if qi < 0:
            rec.update(qi=self.qi)
            out.append((b"", rec, dict(st, cut=0, ratio=self.t)))   # a dropped frame is not a key frame
        else:
            self.enc.cur, self.enc.key = self.cur, self.key
            self.enc.forced = (key, st)
            r = self.enc.frame(planes, qi, dups=dups)
            if key:
                self.key = f
            self.qi = qi
            rec.update(qi=qi)
            rec.update(self.ctl.coded(key, qi, 8 * len(r["packet"])))
            out.append((r["packet"], rec, r["cut"]))
        self.cur = f
        for _ in range(dups):
            self.cur += 1
            d = self.ctl.dup()
            out.append((b"", dict(d, qi=self.qi, duplicate=1), dict(NO_STATS, ratio=self.t)))
        return out


# ---- content ------------------------------------------------------------------------------------------------------------------
def scene(w, h, fmt, n, cut, seed=0):
    """enc_inter_ref's pan that cuts to the pan over another picture (seed + 11) at frame `cut`: both scenes predict well, the cut does
    not."""
    a = enc_inter_ref.sequence("pan", w, h, fmt, n, seed)
    b = enc_inter_ref.sequence("pan", w, h, fmt, n, seed + 11)
    return [a[f] if f < cut else b[f] for f in range(n)]


def flat_noise(w, h, fmt, n, sigma, seed=0):
    """100 plus rounded Gaussian noise of that sigma, fresh every frame, in every plane: prediction never pays (P about I) and
    nothing is worth a key frame."""
    hd, vd = int(not (fmt & 1)), int(not (fmt & 2))
    rng = np.random.default_rng(seed)
    shapes = [(h, w), (h >> vd, w >> hd), (h >> vd, w >> hd)]
    return [[np.clip(100 + np.rint(rng.normal(0.0, sigma, s)), 0, 255).astype(np.uint8) for s in shapes] for _ in range(n)]


def clip(kind, w, h, fmt, n, seed=0, cut=3):
    if kind == "scene":
        return scene(w, h, fmt, n, cut, seed)
    if kind == "flat_noise":
        return flat_noise(w, h, fmt, n, 2, seed)
    return enc_inter_ref.sequence(kind, w, h, fmt, n, seed)
