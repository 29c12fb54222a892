"""enc_rate_ref.py -- TEST INFRASTRUCTURE: a restatement of th_encode_*'s bitrate mode (include/theoraenc_hip.h, "Bitrate mode") in
numpy: the probe E[q] and the controller, to compare the library's choices with exactly.

The packets at a chosen qi are tests/enc_ref.py's (key frames) and tests/enc_inter_ref.py's (inter frames); the transform and the
quantiser are the oracle's.  The probe's stages are stated in tests/rate_stage_ref.py, one function each; Probe composes them.
"""
import numpy as np

import oracle
from tests import enc_ref, enc_inter_ref

from tests import rate_stage_ref as RS
from tests.rate_stage_ref import EXTRA_BITS, HG, code_lengths, dc_pred_masked, hist_bits, token_hist   # noqa: F401 -- stated there

DROP_FRAMES, CAP_OVERFLOW, CAP_UNDERFLOW = 1, 2, 4


class Probe:
    """E[q] of frames of one geometry (the probe of thip_rate.h): tests/rate_stage_ref.py's stages, composed."""

    def __init__(self, fw, fh, fmt, pic, setup):
        self.fw, self.fh, self.fmt, self.pic, self.setup = fw, fh, fmt, pic, setup
        self.geo = enc_inter_ref.Geometry(fw, fh, fmt)
        self.lens = code_lengths(setup)
        self.steps = RS.steps_of(setup)
        self.lam = self.steps[3, :, 1].astype(np.int64)   # the inter luma step at zig-zag index 1

    def _src(self, planes):
        return [np.flipud(a).astype(np.int64) for a in enc_ref.frame_planes(planes, self.fw, self.fh, self.fmt, self.pic)]

    def key(self, planes):
        return RS.probe(self.geo, RS.coef_key(self.geo, self._src(planes)), self.steps, self.lens, False)

    def inter(self, planes, ref):
        """ref: the reference (three planes, bitstream row order, the decoder's PREV)."""
        src = self._src(planes)
        _, mvx, mvy, s0, si, smv = search_stats(src[0], ref[0])
        coef = RS.coef_inter(self.geo, src, ref, mvx, mvy)
        return RS.probe(self.geo, coef, self.steps, self.lens, True, RS.pack_stats(s0, smv, si, mvx, mvy), self.lam)


def search_stats(src, ref):
    """enc_inter_ref.search_stats, the five-mode search before its decision, in motion_search's order: (None, mvx, mvy, S0, SI, Smv),
    the half-pel vector of every macro block whatever its mode."""
    return (None,) + tuple(enc_inter_ref.search_stats(src, ref))


class Controller:
    """The controller of theoraenc_hip.h, step for step (Python integers)."""

    def __init__(self, bitrate, fps, inter, kf_interval, shift, flags=DROP_FRAMES | CAP_OVERFLOW, buffer=None):
        self.bitrate, self.fps, self.inter, self.K, self.shift = bitrate, fps, inter, kf_interval, shift
        self.flags, self.buffer = flags, buffer
        self.started = False
        self.c = [65536, 65536]
        self.L = [None, None]

    def _targets(self):
        self.T = min(max(self.bitrate * self.fps[1] // self.fps[0], 32), 1 << 40)
        self.R = self.T * self.D
        self.Fstar = self.R // 2

    def _caps(self):
        if self.flags & CAP_OVERFLOW:
            self.F = min(self.F, self.R)
        if self.flags & CAP_UNDERFLOW:
            self.F = max(self.F, 0)

    def set_bitrate(self, b):
        self.bitrate = b
        if self.started:
            self._targets()
            self.F = min(self.F, self.R)

    def set_buffer(self, d):
        """TH_ENCCTL_SET_RATE_BUFFER: D clamped to [12, 256]; mid-stream R and F* follow and F = min(F, R)."""
        self.buffer = min(max(d, 12), 256)
        if self.started:
            self.D = self.buffer
            self._targets()
            self.F = min(self.F, self.R)
        return self.buffer

    def choose(self, E, key, f, keypos, first, lastkey, dups):
        """-> (qi or -1 to drop, record)."""
        if not self.started:
            self.D = self.buffer or min(max(self.K if self.inter else 1, 12), 256)
            self._targets()
            self.F = self.Fstar
            self.started = True
        t = 0 if key else 1
        E = [int(x) for x in E]
        self.L[t] = E
        nk = sum(1 for m in range(f + 1, f + self.D) if not self.inter or (m - keypos) % self.K == 0)
        ni = self.D - 1 - nk
        cur, fut = [], []
        for q in range(64):
            cur.append(E[q] * self.c[t] >> 16)
            kt = self.L[0][q] * self.c[0] >> 16 if self.L[0] else None
            it = self.L[1][q] * self.c[1] >> 16 if self.L[1] else None
            if it is None:
                it = kt // 4
            if kt is None:
                kt = 4 * it
            fut.append(nk * kt + ni * it)
        S = self.F + self.D * self.T - self.Fstar
        qi = max([q for q in range(64) if cur[q] + fut[q] <= S], default=0)
        drop = bool(self.flags & DROP_FRAMES) and not first and self.F + self.T - cur[0] < 0 and lastkey >= 0 and \
            f - lastkey + dups < (1 << self.shift)
        rec = dict(fullness_before=self.F, spend=S, estimate=cur[qi], target=self.T, dropped=int(drop))
        if drop:
            self.F += self.T
            self._caps()
            rec.update(fullness_after=self.F, corr=list(self.c))
            return -1, rec
        self.E = E
        return qi, rec

    def coded(self, key, qi, A):
        t = 0 if key else 1
        self.F += self.T - A
        self._caps()
        self.c[t] = min(max((self.c[t] + (A << 16) // max(self.E[qi], 1)) // 2, 4096), 1 << 20)
        return dict(fullness_after=self.F, corr=list(self.c), actual=A)

    def dup(self):
        if not self.started:
            return None
        before = self.F
        self.F += self.T
        self._caps()
        return dict(fullness_before=before, fullness_after=self.F)


class RateStream:
    """The stream th_encode_* makes in bitrate mode: frame(planes, dups) -> list of (packet, record) (the frame's, then its
    duplicates')."""

    def __init__(self, fw, fh, fmt, pic, setup, bitrate, fps=(30, 1), inter=False, kf_interval=64, shift=6, flags=DROP_FRAMES |
                 CAP_OVERFLOW, buffer=None):
        self.enc = enc_inter_ref.InterEncoder(fw, fh, fmt, pic, setup, kf_interval if inter else 1, shift)
        self.probe = Probe(fw, fh, fmt, pic, setup)
        self.ctl = Controller(bitrate, fps, inter, kf_interval, shift, flags, buffer)
        self.inter, self.K, self.shift = inter, kf_interval, shift
        self.cur, self.key, self.qi = -1, -1, 0

    def close(self):
        self.enc.close()

    def frame(self, planes, dups=0):
        f = self.cur + 1
        off = f - self.key
        key = not self.inter or self.key < 0 or off >= self.K or off + dups >= (1 << self.shift)
        if key:
            E = self.probe.key(planes)
        else:
            E = self.probe.inter(planes, [self.enc.ost.get_plane(oracle.FRAME_PREV, p) for p in range(3)])
        qi, rec = self.ctl.choose(E, key, f, f if key else self.key, self.cur < 0, self.key, dups)
        rec.update(probe=list(E), key=int(key and qi >= 0))
        out = []
        if qi < 0:
            rec.update(qi=self.qi)
            out.append((b"", rec))
        else:
            # the restated encoders decide key / inter by their own counters: keep them in step with the drops
            self.enc.cur, self.enc.key = self.cur, self.key
            r = self.enc.frame(planes, qi, dups=dups)
            assert r["key"] == key
            if key:
                self.key = f
            self.qi = qi
            rec.update(qi=qi)
            rec.update(self.ctl.coded(key, qi, 8 * len(r["packet"])))
            out.append((r["packet"], rec))
        self.cur = f
        for _ in range(dups):
            self.cur += 1
            d = self.ctl.dup()
            out.append((b"", dict(d, qi=self.qi, duplicate=1)))
        return out
