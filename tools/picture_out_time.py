"""k_picture_out (thip_picture_out) on the device: HIP events around --iters launches after warm-up, 1080p and 4K, batches of 1 and 4,
every format; algorithmic bytes (the source samples the rectangle needs + the output written) and their share of the 8 TB/s
HBM roofline.  Then one end-to-end comparison at 1080p through th_decode_*: the plain loop with ycbcr_out (every frame copied to
the host), against the same loop with host output off and an RGBA picture on the device per frame.

  python tools/picture_out_time.py [--iters 200] [--e2e-frames 64] [--json out.json] [--skip-e2e]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8.0e12   # bytes/s, MI355X HBM3E peak (spec)
SIZES = {"1080p": (1920, 1088, (0, 0, 1920, 1080)), "4k": (3840, 2160, None)}
FORMATS = [("ycbcr", "linear"), ("rgb", "linear"), ("rgba", "linear"), ("rgba", "nearest"), ("rgb_planar", "linear")]


def algorithmic_bytes(fmt, w, h, x=0, y=0):
    """Source samples the picture needs (4:2:0) + bytes written."""
    cw = ((x + w + 1) >> 1) - (x >> 1)
    ch = ((y + h + 1) >> 1) - (y >> 1)
    src = w * h + 2 * cw * ch
    out = {"ycbcr": src, "rgb": 3 * w * h, "rgba": 4 * w * h, "rgb_planar": 3 * w * h}[fmt]
    return src + out


def kernel_times(args):
    import torch
    import theora_amd
    from theora_amd import _lib
    L = _lib.load()
    rows = []
    rng = np.random.default_rng(1)
    s = torch.cuda.Stream()
    for size, (fw, fh, rect) in SIZES.items():
        for batch in (1, 4):
            states = []
            for i in range(batch):
                st = theora_amd.State(fw, fh)
                for pli in range(3):
                    g = st.planes[pli]
                    st.write_plane(0, pli, rng.integers(16, 236, (g["height"], g["width"]), dtype=np.uint8))
                st.set_ref_idx(0, 0, 0)
                states.append(st)
            x, y, w, h = rect if rect else (0, 0, fw, fh)
            for fmt, chroma in FORMATS:
                shp = theora_amd.picture_shapes(fmt, w, h, x, 0, y)
                outs = [[torch.empty(p, dtype=torch.uint8, device="cuda") for p in shp] if fmt == "ycbcr"
                        else torch.empty(shp, dtype=torch.uint8, device="cuda") for _ in states]
                reqs = (_lib.PictureReq * batch)()
                for i, st in enumerate(states):
                    ptrs, pitches = theora_amd._pic_dst(fmt, outs[i], shp)
                    r = reqs[i]
                    r.state, r.bufi = st.handle, -1
                    r.format, r.chroma = theora_amd.PIC_FORMATS[fmt], theora_amd.CHROMA_MODES[chroma]
                    r.x, r.y, r.width, r.height = (x, y, w, h) if rect else (0, 0, 0, 0)
                    for p in range(3):
                        r.dst[p], r.dst_pitch[p] = ptrs[p], pitches[p]
                h_s = s.cuda_stream
                for _ in range(20):
                    _lib.check(L.thip_picture_out(reqs, batch, h_s), "thip_picture_out")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(args.iters):
                    L.thip_picture_out(reqs, batch, h_s)
                e1.record(s)
                e1.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / args.iters
                nbytes = batch * algorithmic_bytes(fmt, w, h, x, y)
                rows.append(dict(size=size, batch=batch, format=fmt, chroma=chroma, us_per_launch=round(us, 2),
                                 algorithmic_MB=round(nbytes / 1e6, 2), TB_s=round(nbytes / us / 1e6, 3),
                                 roofline_fraction=round(nbytes / ROOF / (us * 1e-6), 3)))
                print(json.dumps(rows[-1]), flush=True)
            for st in states:
                st.close()
    return rows


def e2e(args):
    """1080p th_decode_* plain loop: ycbcr_out per frame vs host output off + an RGBA picture on the device per frame."""
    import torch
    from tests import streamgen
    from theora_amd.decoder import Decoder
    w, h = 1920, 1088
    st = streamgen.Stream(w, h, 0, seed=99)
    pkts = [st.frame(0 if f == 0 else 1, density=0.5)[0] for f in range(8)]   # an intra frame, then inter frames: replayable
    hdr = st.header_packets()
    res = {}
    for mode in ("ycbcr_out", "device_rgba"):
        dec = Decoder(hdr)
        out = None
        if mode == "device_rgba":
            dec.set_host_output(False)
            out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()

        def step(p):
            dec.packetin(p)
            if mode == "ycbcr_out":
                dec.ycbcr_out()
            else:
                dec.picture("rgba", "linear", crop=False, stream=s, out=out)
        for p in pkts:   # warm-up
            step(p)
        torch.cuda.synchronize()
        n = 0
        t0 = time.perf_counter()
        while n < args.e2e_frames:
            for p in pkts:
                step(p)
                n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[mode] = dict(frames=n, fps=round(n / dt, 1), ms_per_frame=round(1e3 * dt / n, 3))
        print(json.dumps({"e2e_1080p": mode, **res[mode]}), flush=True)
        dec.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--e2e-frames", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-e2e", action="store_true", help="kernel timings only (e.g. under rocprofv3)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("picture_out_time: no GPU (the numbers are device times; there is nothing to measure here)")
    out = dict(kernels=kernel_times(args), e2e=None if args.skip_e2e else e2e(args))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
