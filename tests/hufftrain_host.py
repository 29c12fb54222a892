"""hufftrain_host.py -- TEST INFRASTRUCTURE: th_encode_*'s Huffman-code arithmetic (theora_amd/csrc/thip_hufftrain.h) replayed on the
host under AddressSanitizer and UBSan by tests/native/hufftrain_host.cpp.  A Steps object collects steps (valid, trees, train); run()
replays them in one process and returns what the program printed for each."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_exe = None


def build(tmp_path_factory):
    """The program, built once a session; skipped only where g++ has no sanitizer runtimes (as tests/ratectl_host.py)."""
    global _exe
    if _exe:
        return _exe
    out = str(tmp_path_factory.mktemp("hufftrain") / "hufftrain_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "theora_amd", "csrc"), os.path.join(ROOT, "tests", "native", "hufftrain_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", out + ".probe"],
                               input="int main(){return 0;}", capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("g++ with sanitizers not usable here: " + probe.stderr[-300:])
        pytest.fail("hufftrain_host does not build: " + r.stderr[-3000:])
    _exe = out
    return out


def _codes_text(codes):
    return " ".join(str(int(x)) for x in np.asarray(codes, np.int64).reshape(-1))


class Steps:
    def __init__(self):
        self.lines = []

    def valid(self, codes):
        self.lines.append("valid " + _codes_text(codes))

    def trees(self, codes):
        self.lines.append("trees " + _codes_text(codes))

    def train(self, hists, start, rounds):
        counts = " ".join(str(int(x)) for h in hists for x in np.asarray(h, np.int64).reshape(-1))
        self.lines.append("train %d %d %s %s" % (rounds, len(hists), _codes_text(start), counts))

    def run(self, exe, tmp_path):
        """-> one dict a step: ok | nbits, bits | rc, the statistics and codes (80, 32, 2)."""
        path = tmp_path / "steps.txt"
        path.write_text("\n".join(self.lines) + "\n")
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout[-300:], r.stderr[-3000:])
        out = []
        for line in r.stdout.splitlines():
            step, *tokens = line.split()
            d = {"step": step}
            for t in tokens:
                k, v = t.split("=")
                d[k] = v if k == "bits" else np.array(v.split(","), np.int64).reshape(80, 32, 2) if k == "codes" else int(v)
            out.append(d)
        assert [d["step"] for d in out] == [l.split()[0] for l in self.lines]
        return out
