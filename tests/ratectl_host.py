"""ratectl_host.py -- TEST INFRASTRUCTURE: th_encode_*'s rate controllers (theora_amd/csrc/thip_ratectl.h) replayed on the host under
AddressSanitizer and UBSan by tests/native/ratectl_host.cpp, and the same steps through the restatements: tests/enc_rate_ref.py's
Controller, tests/enc_2pass_ref.py's Controller2 and pass-file functions.

A Model is written step by step (bitrate, frame, dup, out, feed ...); every step adds a line to the scenario and the line the
program must print for it, with the frame counters th_encode_ycbcr_in and th_encode_packetout keep.  run() replays the scenario
and compares every field of every line, exactly."""
import copy
import os
import subprocess

import pytest

from tests import enc_2pass_ref as TP
from tests import enc_rate_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTFORMAT = -10, -21
_exe = None


def build(tmp_path_factory):
    """The program, built once a session; skipped only where g++ has no sanitizer runtimes (as tests/test_frontend_fuzz.py)."""
    global _exe
    if _exe:
        return _exe
    out = str(tmp_path_factory.mktemp("ratectl") / "ratectl_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "theora_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ratectl_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", out + ".probe"],
                               input="int main(){return 0;}", capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("g++ with sanitizers not usable here: " + probe.stderr[-300:])
        pytest.fail("ratectl_host does not build: " + r.stderr[-3000:])
    _exe = out
    return out


def _parse(line):
    step, *tokens = line.split()
    d = {}
    for t in tokens:
        k, v = t.split("=")
        d[k] = (b"" if v == "-" else bytes.fromhex(v)) if k == "bytes" else [int(x) for x in v.split(",")] if "," in v else int(v)
    return step, d


def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


class Model:
    def __init__(self, fw=64, fh=48, pic=None, fmt=0, fps=(30, 1), shift=6, inter=False, K=1, quality=0):
        pic = pic or (0, 0, fw, fh)
        self.fields = TP.fields_of(fw, fh, pic, fmt, fps, shift, inter)
        self.fps, self.shift, self.inter, self.K, self.quality = fps, shift, inter, K, quality
        self.lines = ["stream " + " ".join(str(x) for x in self.fields + [K]), "quality %d" % quality]
        self.want = []
        self.ctl = RR.Controller(0, fps, inter, K, shift)
        self.rate, self.cur, self.lastkey, self.qi, self.dups_left, self.is_done = False, -1, -1, 0, 0, False
        # thip_enc_rate_stats and thip_enc_2pass_stats: all 0 before the first packet
        self.st = dict(qi=0, dropped=0, key=0, duplicate=0, target=0, fullness_before=0, fullness_after=0, spend=0, estimate=0,
                       actual=0, probe=[0] * 64, corr=[0, 0])
        self.tp = dict(tp_pass=0, tp_type=0, tp_frame=0, tp_qi=0, budget_left=0, recorded_left=0, recorded=[0] * 64, fresh=[0] * 64,
                       tp_corr=[0] * 4, frames=0, dups=0, A=0)
        # two-pass: the pass, pass 1's records and the one ready to be read, pass 2's file, header and controller
        self.pass_, self.records, self.ready, self.final = 0, [], None, False
        self.file, self.hdr, self.c2 = bytearray(), None, None

    # ---- what the program prints after a packet or a setting -------------------------------------------------------------------
    def _state(self, step):
        c = self.ctl
        d = dict(cur=self.cur, lastkey=self.lastkey, frame_qi=self.qi, bitrate=c.bitrate, flags=c.flags, buf=c.buffer or 0,
                 started=int(c.started), c=list(self.c2.c if self.c2 else c.c))
        d.update((k, getattr(c, k, 0)) for k in ("T", "D", "R", "Fstar", "F"))
        d.update(copy.deepcopy(self.st))
        d.update(copy.deepcopy(self.tp))
        self.want.append((step, d))

    def _start(self):
        """The controller's first frame (pass 2 starts it too, and uses its T alone)."""
        c = self.ctl
        if not c.started:
            c.D = c.buffer or _clamp(self.K if self.inter else 1, 12, 256)
            c._targets()
            c.F = c.Fstar
            c.started = True

    # ---- the settings ------------------------------------------------------------------------------------------------------------
    def bitrate(self, b):
        self.lines.append("bitrate %d" % b)
        self.rate = True
        self.ctl.set_bitrate(b)
        if self.c2:
            self.c2.bitrate = b
        self._state("bitrate")

    def buffer(self, d):
        self.lines.append("buffer %d" % d)
        self.ctl.set_buffer(d)
        self._state("buffer")

    def flags(self, f):
        self.lines.append("flags %d" % f)
        self.ctl.flags = f & 7
        self._state("flags")

    # ---- packets -----------------------------------------------------------------------------------------------------------------
    def _packet(self, rtype, bits, E):
        """Every packet: thip_enc_2pass_stats, and in pass 1 the record."""
        self.tp.update(tp_pass=self.pass_, tp_frame=self.cur, tp_qi=self.qi)
        if self.pass_ == 0:
            return
        self.tp.update(fresh=[0] * 64 if rtype == TP.DUP else list(E))
        if self.pass_ == 2:
            if rtype == TP.DUP:
                self.tp.update(tp_type=TP.DUP, recorded=[0] * 64)
            self.tp.update(budget_left=self.c2.B - self.c2.A, tp_corr=list(self.c2.c) + list(self.c2.ratio), A=self.c2.A)
            return
        self.ready = TP.pack_record(rtype, self.qi, 8 * (bits // 8), [0] * 64 if rtype == TP.DUP else E)
        self.records.append(TP.unpack_record(self.ready))
        dups = sum(r["type"] == TP.DUP for r in self.records)
        self.tp.update(tp_type=rtype, recorded=self.records[-1]["E"], frames=len(self.records) - dups, dups=dups)

    def frame(self, E, dups=0, mul=1, add=0, key=None):
        """A frame probed as E whose packet takes mul x E[qi] + add bits, with `dups` duplicates asked for it -> the qi (-1: dropped;
        None: refused).  key: its type, where it is not to be the interval rule's."""
        E = [int(x) for x in E]
        f = self.cur + 1
        off = f - self.lastkey
        if key is None:
            key = not self.inter or self.lastkey < 0 or off >= self.K or off + dups >= (1 << self.shift)
        self.lines.append("frame %d %d %d %d " % (key, dups, mul, add) + " ".join(str(x) for x in E))
        if self._gate():
            self.want.append(("frame", dict(refused=EINVAL)))
            return None
        if not self.rate:
            self.qi = self.quality
        qi, rtype = self.qi, None
        if self.pass_ == 2:
            rec = TP.unpack_record(bytes(self.file[TP.HEADER_BYTES + f * TP.RECORD_BYTES:TP.HEADER_BYTES + (f + 1) * TP.RECORD_BYTES]))
            key = rec["type"] == TP.KEY or not self.inter or self.lastkey < 0 or f - self.lastkey + dups >= (1 << self.shift)
            self._start()
            c2 = self.c2
            qi = c2.choose(rec, E, key)
            left = c2.B - c2.A
            self.st.update(qi=qi, dropped=0, key=int(key), duplicate=0, target=c2.T, fullness_before=left, spend=left,
                           estimate=c2.cur[qi], probe=E)
            self.tp.update(tp_type=rec["type"], recorded=rec["E"], recorded_left=c2.left_recorded)
        elif self.rate:
            qi, r = self.ctl.choose(E, key, f, f if key else self.lastkey, self.cur < 0, self.lastkey, dups)
            self.st.update(qi=self.qi if qi < 0 else qi, dropped=r["dropped"], key=int(key and qi >= 0), duplicate=0, target=r["target"],
                           fullness_before=r["fullness_before"], spend=r["spend"], estimate=r["estimate"], actual=0, probe=E)
            if qi < 0:
                self.st.update(fullness_after=r["fullness_after"], corr=r["corr"])
                rtype = TP.DROPPED
        self.cur, self.dups_left, bits = f, dups, 0
        if rtype is None:
            rtype = TP.KEY if key else TP.INTER
            self.qi, bits = qi, mul * E[qi] + add
            if key:
                self.lastkey = f
            if self.pass_ == 2:
                self.c2.coded(key, qi, bits)
                self.st.update(actual=bits, fullness_after=self.c2.B - self.c2.A, corr=list(self.c2.c))
            elif self.rate:
                self.st.update(self.ctl.coded(key, qi, bits))
        self._packet(rtype, bits, E)
        self._state("frame")
        return -1 if rtype == TP.DROPPED else qi

    def dup(self):
        self.lines.append("dup")
        if self.cur >= 0:
            self.cur += 1
            self.dups_left = max(self.dups_left - 1, 0)
        d = self.ctl.dup() if self.rate else None
        if d:
            self.st.update(d, dropped=0, key=0, duplicate=1, qi=self.qi, spend=0, estimate=0, actual=0, probe=[0] * 64)
            if self.pass_ == 2:
                self.st.update(fullness_before=self.c2.B - self.c2.A, fullness_after=self.c2.B - self.c2.A)
        if self.cur >= 0:
            self._packet(TP.DUP, 0, [0] * 64)
        self._state("dup")

    def done(self):
        self.lines.append("done")
        self.is_done = True

    # ---- the pass file -----------------------------------------------------------------------------------------------------------
    def out(self):
        """TH_ENCCTL_THIP_2PASS_OUT -> the bytes expected."""
        self.lines.append("out")
        data = b""
        if self.pass_ == 0:
            self.pass_ = self.tp["tp_pass"] = 1
            data = TP.pack_header(self.fields)
        elif self.ready is not None:
            data, self.ready = self.ready, None
        elif self.is_done and not self.final:
            self.final = True
            data = TP.finish_header(self.fields, self.records)
        self.want.append(("out", dict(n=len(data), bytes=data)))
        return data

    def _n(self):
        return self.cur + 1 + self.dups_left

    def _wanted(self):
        return TP.wanted(len(self.file), self.hdr, self._n())

    def _gate(self):
        if self.pass_ != 2:
            return 0
        return EINVAL if self.hdr is None or self.cur + 1 >= self.hdr["frames"] + self.hdr["dups"] or self._wanted() > 0 else 0

    def _in_line(self, step, rc):
        h = self.hdr or dict(frames=0, dups=0)
        self.tp.update(tp_pass=self.pass_, frames=h["frames"], dups=h["dups"])
        self.want.append((step, dict(rc=rc, tp_pass=self.pass_, stats_pass=self.pass_, hdr_ok=int(self.hdr is not None),
                                     have=len(self.file), frames=h["frames"], dups=h["dups"])))
        return rc

    def feed(self, data):
        """TH_ENCCTL_THIP_2PASS_IN with bytes -> the answer expected."""
        self.lines.append("in " + (data.hex() or "-"))
        self.pass_, used, rc = 2, 0, None
        if self.hdr is None:
            used = min(len(data), TP.HEADER_BYTES - len(self.file))
            self.file += data[:used]
            try:
                h = TP.unpack_header(bytes(self.file))
                if h["fields"] != self.fields:
                    rc = EINVAL
                else:
                    self.hdr = h
                    self.c2 = TP.Controller2(self.ctl.bitrate, self.fps, h)
            except TP.NotFormat:
                rc = ENOTFORMAT
            except TP.Truncated:
                return self._in_line("in", used)
            if rc is not None:   # refused: as before the first byte
                self.file, self.pass_ = bytearray(), 0
                return self._in_line("in", rc)
        total = TP.HEADER_BYTES + (self.hdr["frames"] + self.hdr["dups"]) * TP.RECORD_BYTES
        take = min(len(data) - used, total - len(self.file))
        self.file += data[used:used + take]
        return self._in_line("in", used + take)

    def wanted(self):
        """TH_ENCCTL_THIP_2PASS_IN(NULL)."""
        self.lines.append("want")
        self.pass_ = 2
        return self._in_line("want", self._wanted())

    def gate(self):
        self.lines.append("gate")
        self.want.append(("gate", dict(rc=self._gate())))
        return self._gate()

    # ---- the replay --------------------------------------------------------------------------------------------------------------
    def run(self, exe, tmp_path):
        """Replays the scenario; every field of every line must be the restatement's.  -> the lines as (step, dict)."""
        path = tmp_path / "scenario.txt"
        path.write_text("\n".join(self.lines) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
        got = [_parse(l) for l in r.stdout.splitlines()]
        assert len(got) == len(self.want)
        for n, (g, w) in enumerate(zip(got, self.want)):
            assert g[0] == w[0] and sorted(g[1]) == sorted(w[1]), (n, g[0], w[0], sorted(set(g[1]) ^ set(w[1])))
            for k in w[1]:
                assert g[1][k] == w[1][k], "line %d (%s), %s: the library's %r, the restatement's %r" % (n, g[0], k, g[1][k], w[1][k])
        return got
