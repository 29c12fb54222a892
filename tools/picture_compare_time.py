"""k_picture_compare (thip_picture_compare) on the device, for 1080p and 4K at 4:2:0, with THIP_CMP_SSE alone and with
THIP_CMP_SSIM as well.  A call is the 96-byte memset of the result and the kernel.  For each case

  (a) graph_us: --iters calls captured once into a HIP graph on a stream (memset node, kernel node, ... in a chain) and replayed:
      the median over --repeats replays of the time between two HIP events around a replay, over --iters.  No host work is inside
      the window, so this is the device's time for a call, launch gaps between the nodes included;
  (b) eager_us / eager_host_us: the same calls made one by one as a program makes them (tools/picture_resize_time.py's median_us:
      events around --iters calls, and the host time of the loop that queued them; where the two are close the host set the pace);
  (c) the bytes read -- both pictures once, 2 x 1.5 bytes a pixel -- over (a), and the byte floor at the HBM rate of
      profiles/r03_hbm_ceiling.txt (6.71 TB/s);
  (d) what a user does today on the device: State.picture("ycbcr") of the picture region, then per plane a torch squared-difference
      sum (int32 difference, int64 sum), checked equal to the kernel's sse before it is timed (eager, like (b)).

The kernel alone, without the memset and the gaps, is a `rocprofv3 --kernel-trace --stats -- python tools/picture_compare_time.py`
run of its own.

Then the encoder: th_encode_* with the quality statistics on (TH_ENCCTL_THIP_SET_QUALITY_STATS), key frames and inter frames at
quality 32 -- the median compare_ms of TH_ENCCTL_THIP_GET_QUALITY_STATS beside the frame's device time of TH_ENCCTL_THIP_GET_TIMES.

  python tools/picture_compare_time.py [--iters 100] [--repeats 5] [--frames 8] [--jsonl profiles/picture_compare.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.71e12   # bytes/s
SIZES = {"1080p": (1920, 1088, (0, 0, 1920, 1080)), "4k": (3840, 2160, (0, 0, 3840, 2160))}


def graph_us(stream, fn, iters, repeats):
    """`iters` calls of fn() captured into one graph on `stream`; the median over `repeats` replays of a replay's device time, a call."""
    import statistics
    import torch
    g = torch.cuda.CUDAGraph()
    stream.synchronize()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(iters):
            fn()
    with torch.cuda.stream(stream):
        for _ in range(3):
            g.replay()
        out = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            g.replay()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("picture_compare_time: no GPU (the numbers are device times; there is nothing to measure here)")
    import theora_amd
    from picture_resize_time import median_us
    from theora_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(1)
    s = torch.cuda.Stream()
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
    for name, (fw, fh, rect) in SIZES.items():
        st = theora_amd.State(fw, fh)
        for pli in range(3):
            g = st.planes[pli]
            st.write_plane(0, pli, rng.integers(16, 236, (g["height"], g["width"]), dtype=np.uint8))
        st.set_ref_idx(0, 0, 0)
        x, y, w, h = rect
        shapes = theora_amd.picture_shapes("ycbcr", w, h, x, 0, y)
        ref = [torch.from_numpy(rng.integers(16, 236, sh, dtype=np.uint8)).cuda() for sh in shapes]
        nbytes = 2 * sum(sh[0] * sh[1] for sh in shapes)
        res = torch.zeros(12, dtype=torch.int64, device="cuda")

        def today():
            planes = st.picture("ycbcr", rect=rect, stream=s)
            return [((a.to(torch.int32) - b.to(torch.int32)) ** 2).sum(dtype=torch.int64) for a, b in zip(planes, ref)]
        with torch.cuda.stream(s):
            want = [int(v.item()) for v in today()]
        today_us, today_host_us = median_us(s, today, args.iters, args.repeats)
        for metrics in (("sse",), ("sse", "ssim")):
            r = _lib.PictureCompareReq()
            r.state, r.bufi, r.flags = st.handle, -1, theora_amd._cmp_flags(metrics)
            r.x, r.y, r.width, r.height = rect
            for p in range(3):
                r.ref[p], r.ref_pitch[p] = ref[p].data_ptr(), ref[p].stride(0)
            r.result = res.data_ptr()
            _lib.check(L.thip_picture_compare(r, 1, s.cuda_stream), "thip_picture_compare")
            s.synchronize()
            assert res[:3].tolist() == want, (res.tolist(), want)
            def call():
                _lib.check(L.thip_picture_compare(r, 1, s.cuda_stream), "thip_picture_compare")
            us, host_us = median_us(s, call, args.iters, args.repeats)
            gus = graph_us(s, call, args.iters, args.repeats)
            s.synchronize()
            assert res[:3].tolist() == want                      # the replays made the same sums
            floor = nbytes / HBM * 1e6
            emit(dict(case="%s_%s" % (name, "+".join(metrics)), graph_us=round(gus, 2), eager_us=round(us, 2),
                      eager_host_us=round(host_us, 2), MB_read=round(nbytes / 1e6, 2), GBps=round(nbytes / gus / 1e3, 1),
                      floor_us=round(floor, 2), graph_over_floor=round(gus / floor, 2), today_us=round(today_us, 2),
                      today_host_us=round(today_host_us, 2), eager_over_today=round(us / today_us, 3)))
        st.close()
    # the encoder: compare_ms beside the frame's device time
    from tests import enc_inter_ref
    from theora_amd.encoder import Encoder
    for name, (fw, fh, rect) in SIZES.items():
        frames = [theora_amd_planes(fr, rect) for fr in enc_inter_ref.sequence("pan", fw, fh, 0, args.frames, seed=5)]
        for inter in (False, True):
            for metrics in (("sse",), ("sse", "ssim")):
                e = Encoder(fw, fh, 0, 32, pic=rect, inter=inter, keyframe_interval=args.frames if inter else None)
                e.set_quality_stats(metrics)
                e.header_packets()
                cmp_ms, dev_ms = [], []
                for f, fr in enumerate(frames):
                    e.encode(fr)
                    e.packetout(f == len(frames) - 1)
                    q = e.quality_stats()
                    if f >= 2:
                        cmp_ms.append(q["compare_ms"])
                        dev_ms.append(e.times()[0])
                e.close()
                emit(dict(case="encoder_%s_%s_%s" % (name, "inter" if inter else "key", "+".join(metrics)),
                          compare_ms=round(float(np.median(cmp_ms)), 4), device_ms=round(float(np.median(dev_ms)), 4),
                          compare_over_device=round(float(np.median(cmp_ms) / np.median(dev_ms)), 4)))
    if args.jsonl:
        with open(args.jsonl, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def theora_amd_planes(frame, rect):
    """The picture-sized planes of a frame (4:2:0, even corner)."""
    x, y, w, h = rect
    return [np.ascontiguousarray(frame[0][y:y + h, x:x + w])] + \
           [np.ascontiguousarray(frame[p][y >> 1:(y + h + 1) >> 1, x >> 1:(x + w + 1) >> 1]) for p in (1, 2)]


if __name__ == "__main__":
    main()
