"""k_picture_resize (thip_picture_resize) on the device, after tools/picture_out_time.py: HIP events around --iters launches, the
median of --repeats such runs, for the four cases DESIGN.md 5.13 records:

  4K -> 1080p "ycbcr" area;  1080p -> 720p "ycbcr" area;  1080p -> 224 x 224 planar float16 area, (x - mean) / std;
  1080p -> 1080p "rgb" bilinear (beside k_picture_out's ("rgb", "linear"), measured in the same run)

and for each (a) the kernel's time, (b) its byte floor -- the source rectangle's bytes plus the output bytes at the HBM rate of
profiles/r03_hbm_ceiling.txt (copy 1R:1W, 120 MB: 6.71 TB/s) --, (c) the same tensor made without the kernel: State.picture() at
full size, then torch.nn.functional.interpolate and the dtype / normalise operations on the device.

  python tools/picture_resize_time.py [--iters 100] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.71e12   # bytes/s
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
P1080 = (1920, 1088, (0, 0, 1920, 1080))
CASES = [   # name, (frame w, frame h, rect), output size, format, filter, float16?
    ("4k_to_1080p_ycbcr_area", (3840, 2160, None), (1920, 1080), "ycbcr", "area", False),
    ("1080p_to_720p_ycbcr_area", P1080, (1280, 720), "ycbcr", "area", False),
    ("1080p_to_224_planar_f16_area", P1080, (224, 224), "rgb_planar", "area", True),
    ("1080p_to_1080p_rgb_bilinear", P1080, (1920, 1080), "rgb", "bilinear", False),
]


def median_us(stream, fn, iters, repeats):
    """Medians over `repeats` of the mean time of `iters` calls of fn() queued on `stream`: (between two events on the device, of
    the host loop that queued them).  Where the two are equal the host, not the device, set the pace."""
    import torch
    with torch.cuda.stream(stream):
        for _ in range(10):
            fn()
        dev, host = [], []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(iters):
                fn()
            e1.record(stream)
            host.append((time.perf_counter() - t0) * 1e6 / iters)
            e1.synchronize()
            dev.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(dev), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("picture_resize_time: no GPU (the numbers are device times; there is nothing to measure here)")
    import theora_amd
    from theora_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(1)
    s = torch.cuda.Stream()
    scale = [1 / (255 * sd) for sd in STD]
    bias = [-m / sd for m, sd in zip(MEAN, STD)]
    mean_t = torch.tensor(MEAN, device="cuda").view(3, 1, 1)
    std_t = torch.tensor(STD, device="cuda").view(3, 1, 1)
    rows = []
    for name, (fw, fh, rect), size, fmt, filt, f16 in CASES:
        st = theora_amd.State(fw, fh)
        for pli in range(3):
            g = st.planes[pli]
            st.write_plane(0, pli, rng.integers(16, 236, (g["height"], g["width"]), dtype=np.uint8))
        st.set_ref_idx(0, 0, 0)
        x, y, w, h = rect if rect else (0, 0, fw, fh)
        dtype = torch.float16 if f16 else torch.uint8
        shp = theora_amd.picture_resize_shapes(fmt, size[0], size[1], 0)
        out = ([torch.empty(p, dtype=dtype, device="cuda") for p in shp] if fmt == "ycbcr" else torch.empty(shp, dtype=dtype, device="cuda"))
        ptrs, pitches = theora_amd._pic_dst(fmt, out, shp, dtype)
        r = _lib.PictureResizeReq()
        r.state, r.bufi = st.handle, -1
        r.format, r.filter, r.elem = theora_amd.PIC_FORMATS[fmt], theora_amd.FILTERS[filt], theora_amd._elem(dtype)
        r.x, r.y, r.width, r.height = (x, y, w, h) if rect else (0, 0, 0, 0)
        r.out_width, r.out_height = size
        for p in range(3):
            r.scale[p], r.bias[p], r.dst[p], r.dst_pitch[p] = scale[p], bias[p], ptrs[p], pitches[p]
        _lib.check(L.thip_picture_resize(r, 1, s.cuda_stream), "thip_picture_resize")
        kernel_us, kernel_host_us = median_us(s, lambda: L.thip_picture_resize(r, 1, s.cuda_stream), args.iters, args.repeats)
        src_bytes = w * h + 2 * (((x + w + 1) >> 1) - (x >> 1)) * (((y + h + 1) >> 1) - (y >> 1))
        out_bytes = sum(t.numel() * t.element_size() for t in (out if fmt == "ycbcr" else [out]))
        floor_us = (src_bytes + out_bytes) / HBM * 1e6

        def without():   # (c): the same tensor shape from the full-size picture and torch operations
            if fmt == "ycbcr":
                planes = st.picture("ycbcr", rect=rect, stream=s)
                return [F.interpolate(p[None, None].float(), size=tuple(o.shape), mode="area").round_().to(torch.uint8)[0, 0]
                        for p, o in zip(planes, out)]
            if f16:
                full = st.picture("rgb_planar", "linear", rect=rect, stream=s)
                small = F.interpolate(full[None].float(), size=(size[1], size[0]), mode="area")[0]
                return ((small / 255 - mean_t) / std_t).half()
            return L.thip_picture_out(q, 1, s.cuda_stream)   # the same size: k_picture_out alone, into the same tensor
        if fmt == "rgb":
            q = _lib.PictureReq()
            q.state, q.bufi, q.format, q.chroma = st.handle, -1, _lib.PIC_RGB24, _lib.CHROMA_LINEAR
            q.x, q.y, q.width, q.height = x, y, w, h
            q.dst[0], q.dst_pitch[0] = ptrs[0], pitches[0]
        without_us, without_host_us = median_us(s, without, args.iters, args.repeats)
        rows.append(dict(case=name, kernel_us=round(kernel_us, 2), floor_us=round(floor_us, 2), without_us=round(without_us, 2),
                         kernel_host_us=round(kernel_host_us, 2), without_host_us=round(without_host_us, 2),
                         MB=round((src_bytes + out_bytes) / 1e6, 2), kernel_over_floor=round(kernel_us / floor_us, 2),
                         kernel_over_without=round(kernel_us / without_us, 3)))
        print(json.dumps(rows[-1]), flush=True)
        st.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
