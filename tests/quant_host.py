"""quant_host.py -- TEST INFRASTRUCTURE: th_encode_*'s quantisation-parameter code (theora_amd/csrc/thip_quant.h) replayed on the host
under AddressSanitizer and UBSan by tests/native/quant_host.cpp.  A Steps object collects parameter sets; run() replays them in one
child process and returns what the program printed for each.  Nothing goes into LD_PRELOAD: the program is linked with the
sanitizers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_exe = None


def build(tmp_path_factory):
    """The program, built once a session; skipped only where g++ has no sanitizer runtimes (as tests/hufftrain_host.py)."""
    global _exe
    if _exe:
        return _exe
    out = str(tmp_path_factory.mktemp("quant") / "quant_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "theora_amd", "csrc"), os.path.join(ROOT, "tests", "native", "quant_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", out + ".probe"],
                               input="int main(){return 0;}", capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("g++ with sanitizers not usable here: " + probe.stderr[-300:])
        pytest.fail("quant_host does not build: " + r.stderr[-3000:])
    _exe = out
    return out


class Steps:
    def __init__(self):
        self.lines = []

    def set(self, p, null=()):
        """A tests/enc_quant_ref.Params (valid or not; at most 64 sizes a (qti, pli)); null: the (qti, pli) whose arrays are NULL."""
        t = [str(v) for v in list(p.dc) + list(p.ac) + list(p.lf)]
        for qti in range(2):
            for pli in range(3):
                sizes, mats = list(p.sizes[qti][pli]), np.asarray(p.mats[qti][pli]).reshape(-1, 64)
                if (qti, pli) in null:
                    t += [str(len(sizes)), "0"]
                    continue
                t += [str(len(sizes)), "1"] + [str(v) for v in sizes] + [str(int(v)) for v in mats[:len(sizes) + 1].reshape(-1)]
                assert len(mats) == len(sizes) + 1 and len(sizes) <= 64
        self.lines.append("set " + " ".join(t))

    def run(self, exe, tmp_path):
        """-> one dict a step: valid and, where valid, nbms, bits, again, steps_ok, floor (6, 64)."""
        path = tmp_path / "steps.txt"
        path.write_text("\n".join(self.lines) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
        out = []
        for line in r.stdout.splitlines():
            step, *tokens = line.split()
            d = {"step": step}
            for tok in tokens:
                k, v = tok.split("=")
                d[k] = v if k == "bits" else np.array(v.split(","), np.int64).reshape(6, 64) if k == "floor" else int(v)
            out.append(d)
        assert len(out) == len(self.lines)
        return out
