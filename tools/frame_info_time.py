"""k_frame_info (thip_frame_info_out) on the device, after tools/picture_resize_time.py: device events around
replays of a captured graph of --iters launches (plain back-to-back launches where capture is refused), the median of --repeats,
at 1080p and 4K for

  maps      the three fragment maps kind, mv and ncoef of all three planes
  flow_f16  the dense field in float16        flow_f32  in float32        valid  the uint8 plane

each from a caller's frag_info of a "mixed" synthetic frame.  The destinations rotate over enough buffers to exceed the 256 MB
Infinity Cache, so that the stores go to HBM.  Beside each time its byte floor: the bytes written plus the command words read (8
bytes a tile position: the kernel reads word0, the line brings word1) at the HBM rate of profiles/r03_hbm_ceiling.txt (6.71 TB/s).

  python tools/frame_info_time.py [--iters 50] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.71e12   # bytes/s
SIZES = {"1080p": (1920, 1088), "4k": (3840, 2160)}
CASES = {"maps": ("kind", "mv", "ncoef"), "flow_f16": ("flow",), "flow_f32": ("flow",), "valid": ("valid",)}


def timed(stream, launches, iters, repeats):
    """Median device time in microseconds of one launch: `launches` (a list of callables, one per rotating destination) queued
    `iters` times in turn, as one captured graph replayed between two events; (time, "graph" or "launches")."""
    import torch

    def burst():
        for k in range(iters):
            launches[k % len(launches)]()
    how = "graph"
    with torch.cuda.stream(stream):
        burst()
        stream.synchronize()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                burst()
            run = g.replay
        except Exception:
            how, run = "launches", burst
        run()
        stream.synchronize()
        us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(us), min(us), max(us), how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frame_info_time: no GPU (the numbers are device times; there is nothing to measure here)")
    import theora_amd
    from theora_amd import _lib, synth
    L = _lib.load()
    s = torch.cuda.Stream()
    rows = []
    for size, (fw, fh) in SIZES.items():
        geom = synth.Geometry(fw, fh)
        frm = synth.gen_frame(geom, np.random.default_rng(3), theora_amd.INTER_FRAME, "mixed", flimit=4)
        words = torch.from_numpy(synth.pack_frame(geom, frm)["info"].view(np.int32).reshape(-1)).cuda()
        st = theora_amd.State(fw, fh)
        shapes = theora_amd.frame_info_shapes(fw, fh, 0, 0, 0)
        for name, what in CASES.items():
            dtype = torch.float32 if name == "flow_f32" else torch.float16
            one = theora_amd.frame_info_alloc(shapes, what, dtype, "cuda")
            out_bytes = sum(t.numel() * t.element_size() for v in one.values() for t in (v if isinstance(v, list) else [v]))
            nbuf = max(2, min(12, -(-300_000_000 // out_bytes)))
            outs = [one] + [theora_amd.frame_info_alloc(shapes, what, dtype, "cuda") for _ in range(nbuf - 1)]
            reqs = []
            for out in outs:
                r = _lib.FrameInfoReq()
                r.state, r.frag_info, r.refs = st.handle, words.data_ptr(), 3
                for key in ("kind", "mv", "ncoef"):
                    for p, t in enumerate(out.get(key) or ()):
                        getattr(r, key)[p], getattr(r, key + "_pitch")[p] = t.data_ptr(), t.stride(0)
                if "flow" in out:
                    t = out["flow"]
                    r.flow, r.flow_pitch, r.elem = t.data_ptr(), t.stride(1) * t.element_size(), theora_amd._elem(t.dtype)
                if "valid" in out:
                    r.valid, r.valid_pitch = out["valid"].data_ptr(), out["valid"].stride(0)
                reqs.append(r)
            _lib.check(L.thip_frame_info_out(reqs[0], 1, s.cuda_stream), "thip_frame_info_out")
            launches = [(lambda r=r: L.thip_frame_info_out(r, 1, s.cuda_stream)) for r in reqs]
            us, lo, hi, how = timed(s, launches, args.iters, args.repeats)
            # the words the kernel touches: the maps read every plane's, the dense outputs the luma plane's
            read = 8 * 64 * (geom.ntiles if name == "maps" else geom.tiles_x[0] * geom.tiles_y[0])
            floor_us = (out_bytes + read) / HBM * 1e6
            rows.append(dict(size=size, case=name, us=round(us, 2), us_min=round(lo, 2), us_max=round(hi, 2), timed_as=how,
                             rotating_buffers=nbuf, written_MB=round(out_bytes / 1e6, 3), read_MB=round(read / 1e6, 3),
                             floor_us=round(floor_us, 2), over_floor=round(us / floor_us, 2),
                             TB_s=round((out_bytes + read) / us / 1e6, 3)))
            print(json.dumps(rows[-1]), flush=True)
            del outs, reqs, launches, one
            torch.cuda.empty_cache()
        st.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
