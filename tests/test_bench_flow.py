"""bench.py's control flow without a GPU: the device side replaced by stand-ins that decode nothing (so the oracle comparison is
switched off with --no-parity and no number means anything) -- what is checked is that every keyed entry is produced, the line is
valid JSON under the 6 KB the driver's 8 KB tail leaves room for, the detail file is written, and the worker processes deliver.
The real thing runs on the GPU box (tools/prof_round6.sh).
A plain run (no --full) is checked to submit the headline's steps and nothing else."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeState:
    def __init__(self, w, h, fmt=0, device=None):
        self.w, self.h = w, h
        self.frame_bytes = w * h * 3 // 2

    def read_plane(self, bufi, pli):
        return np.zeros((self.h >> (1 if pli else 0), self.w >> (1 if pli else 0)), np.uint8)

    def ref_idx(self, which):
        return 0

    def close(self):
        pass


class _FakePlan:
    submitted = 0
    frames = []         # the frame (index into a stream's [key, inter_1 .. inter_pool]) of every submitted step, in order

    def __init__(self, states, descs):
        assert len(states) == len(descs) and all(d is not None for d in descs)
        self.frame = descs[0]["frame"]

    def submit(self, stream=None):
        _FakePlan.submitted += 1
        _FakePlan.frames.append(self.frame)


def _fake_device(monkeypatch):
    """bench.main() without a GPU: states, plans and uploads are stand-ins; an uploaded frame remembers its index in the pool
    (the file a worker wrote it to ends in _<index>.npz)."""
    sys.path.insert(0, ROOT)
    import torch
    import theora_amd
    from theora_amd import synth
    import bench
    load = bench._npz_load
    monkeypatch.setattr(bench, "_npz_load", lambda p: dict(load(p), _frame=int(p.rsplit("_", 1)[1][:-4])))
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)

    class _S:
        cuda_stream = 0

        def synchronize(self):
            pass
    monkeypatch.setattr(torch.cuda, "Stream", _S)
    monkeypatch.setattr(torch, "device", lambda *a: None)
    monkeypatch.setattr(theora_amd, "State", _FakeState)
    monkeypatch.setattr(theora_amd, "BatchPlan", _FakePlan)
    monkeypatch.setattr(theora_amd, "synchronize", lambda: None)
    monkeypatch.setattr(theora_amd, "profile_reset", lambda: None)
    monkeypatch.setattr(theora_amd, "profile_enable", lambda on: None)
    monkeypatch.setattr(theora_amd, "profile_read", lambda: ([256, 0], [12.5, 0.0]))
    monkeypatch.setattr(synth, "upload_frame", lambda packed, device="cuda": (dict(nslots=packed["nslots"], frame=packed["_frame"]), None))
    return bench


def test_default_line_fits_the_drivers_tail(monkeypatch, tmp_path, capsys):
    bench = _fake_device(monkeypatch)
    detail = tmp_path / "detail.json"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--size", "qcif", "--all-entries", "--no-parity", "--no-cpu-baseline", "--no-pmc", "--no-enc", "--no-e2e",
                                      "--steps", "20", "--repeats", "3", "--min-time", "0", "--detail", str(detail),
                                      "--dump-outputs", str(tmp_path / "dump")])
    bench.main()
    out = capsys.readouterr().out.strip().splitlines()[-1]
    if os.environ.get("THIP_SHOW_LINE"):
        sys.stderr.write("%d bytes: %s\n" % (len(out), out))
    assert len(out) < 6000, len(out)
    line = json.loads(out)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "entries"):
        assert k in line, k
    assert line["steps"] == 20 and line["n_gpus"] == 1 and line["config"]["workload"].startswith("qcif")
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(line["roofline"])
    want = {"4k_smooth", "form_dequant16", "wide_0pct", "wide_1pct", "wide_10pct", "1080p_single_stream", "1080p_four_streams", "720p_single_stream",
            "1080p_single_gop16"}
    assert want <= set(line["entries"]), sorted(want - set(line["entries"]))
    for name in want:
        e = line["entries"][name]
        assert set(("value", "ms_per_step", "frac", "ws_MB", "gt_IC")) <= set(e), (name, e)
    # 16 states x 7 distinct 1080p command streams do not fit the 256 MB Infinity Cache; one 1080p stream's pool does
    assert line["entries"]["1080p_single_gop16"]["gt_IC"] and not line["entries"]["1080p_single_stream"]["gt_IC"]
    d = json.loads(detail.read_text())
    assert d["entries"]["1080p_single_gop16"]["distinct_descriptors"] == 16 * 7
    assert d["line"]["value"] == line["value"] and "wall_s" in d and d["wall_s"]["total"] > 0
    assert _FakePlan.submitted > 1000
    # the last timed step's pictures: three planes of each of the four streams, whole at this size
    dumped = sorted(os.listdir(tmp_path / "dump"))
    assert dumped == sorted("stream%d_%s.npy" % (s, p) for s in range(4) for p in ("y", "cb", "cr")), dumped
    for s in range(4):
        for p, shape in (("y", (144, 176)), ("cb", (72, 88)), ("cr", (72, 88))):
            a = np.load(tmp_path / "dump" / ("stream%d_%s.npy" % (s, p)))
            assert a.dtype == np.float32 and a.shape == shape


def test_plain_run_times_the_headline_only(monkeypatch, tmp_path, capsys):
    """Without --full: the --parity-frames frames (unchecked), the warm-up and the timed steps of the one sequence, nothing else
    submitted; the line holds the headline and nothing that takes a run of its own; no detail file."""
    bench = _fake_device(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--size", "qcif", "--steps", "20", "--warmup", "5", "--dump-outputs", str(tmp_path / "dump")])
    _FakePlan.frames = []
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert _FakePlan.frames == [bench.seq_frame(i, 0, 1, 6) for i in range(40 + 5 + 20)]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "timing", "pipeline", "wall_s"):
        assert k in line, k
    assert line["metric"] == "decode frames/sec (qcif 4:2:0, bit-exact)" and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "i16" and line["steps"] == 20 and line["warmup"] == 5
    assert line["value"] > 0 and line["ms_per_step"] >= 0
    for k in ("roofline", "entries", "cpu_baseline", "parity", "detail"):
        assert k not in line, k
    assert sorted(os.listdir(tmp_path)) == ["dump"]
    assert sorted(os.listdir(tmp_path / "dump")) == sorted("stream%d_%s.npy" % (s, p) for s in range(4) for p in ("y", "cb", "cr"))

def test_dump_outputs_stay_in_budget_and_repeat(tmp_path):
    """bench.dump_arrays: whole arrays in float32 when they fit; else the same seeded sample of every array in every run, the files
    together within the budget."""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(7)
    arrays = {"stream0_y": rng.integers(0, 256, (96, 128), dtype=np.uint8), "stream0_cb": rng.integers(0, 256, (48, 64), dtype=np.uint8)}
    bench.dump_arrays(str(tmp_path / "whole"), arrays)
    for name, a in arrays.items():
        b = np.load(tmp_path / "whole" / (name + ".npy"))
        assert b.dtype == np.float32 and np.array_equal(b, a)
    budget = 8192
    for run in ("first", "second"):
        bench.dump_arrays(str(tmp_path / run), arrays, budget=budget)
        assert sum(os.path.getsize(tmp_path / run / (name + ".npy")) for name in arrays) <= budget
    for name, a in arrays.items():
        b = np.load(tmp_path / "first" / (name + ".npy"))
        assert b.dtype == np.float32 and b.ndim == 1 and 0 < b.size < a.size
        assert np.array_equal(b, np.load(tmp_path / "second" / (name + ".npy")))
        assert set(b.astype(np.uint8).tolist()) <= set(a.reshape(-1).tolist())
