"""k_picture_in (thip_picture_in) on the device: HIP events around --iters launches after warm-up, 1920x1080 and 3840x2160, the three
R'G'B' formats, 4:2:0 and 4:4:4.  Each time stands next to (a) the byte floor -- the bytes the conversion must read and write over
the bandwidth profiles/r03_hbm_ceiling.txt measured for a 2-reads-to-1-write stream (5980 GB/s; 3 or 4 bytes in and 1.5 out a pixel
at 4:2:0 is that mix) -- and (b) the same conversion in plain torch ops on the same tensor in the same process, which is what a
caller writes without the library (checked equal to the kernel's planes before it is timed).  Then the median encode_rgb +
packetout call at 1080p, quality 48, device packetiser on, beside the same frames given as Y'CbCr device tensors.

  python tools/picture_in_time.py [--iters 200] [--enc-frames 48] [--jsonl profiles/picture_in.jsonl] [--skip-enc]
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

BANDWIDTH = 5980.2e9   # bytes/s: profiles/r03_hbm_ceiling.txt, "2R:1W 600.0 MB/launch"
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
FORMATS = ["rgb", "rgba", "rgb_planar"]
PIXEL_FMTS = {"420": 0, "444": 3}


def floor_bytes(fmt, pf, w, h):
    """Bytes the conversion reads (every source byte of the picture, A included) and writes (the three planes)."""
    hdec, vdec = int(not (pf & 1)), int(not (pf & 2))
    cw, ch = (w + hdec) >> hdec, (h + vdec) >> vdec
    return (4 if fmt == "rgba" else 3) * w * h + w * h + 2 * cw * ch


def torch_convert(src, fmt, pf):
    """The definition of include/theora_hip.h in plain torch ops (pic_x = pic_y = 0): what callers do today."""
    import torch
    if fmt == "rgb_planar":
        R, G, B = (src[c].to(torch.int32) for c in range(3))
    else:
        R, G, B = (src[..., c].to(torch.int32) for c in range(3))
    h, w = R.shape
    hdec, vdec = int(not (pf & 1)), int(not (pf & 2))
    Y = 16 + ((16829 * R + 33039 * G + 6416 * B + 32768) >> 16)
    s = hdec + vdec
    if s:
        ys = [torch.clamp(torch.arange((h + vdec) >> vdec, device=src.device) * (1 + vdec) + d, max=h - 1) for d in range(1 + vdec)]
        xs = [torch.clamp(torch.arange((w + hdec) >> hdec, device=src.device) * (1 + hdec) + d, max=w - 1) for d in range(1 + hdec)]
        R, G, B = (sum(c[y][:, x] for y in ys for x in xs) for c in (R, G, B))
    Cb = 128 + ((-9714 * R - 19070 * G + 28784 * B + (1 << (15 + s))) >> (16 + s))
    Cr = 128 + ((28784 * R - 24103 * G - 4681 * B + (1 << (15 + s))) >> (16 + s))
    return [p.to(torch.uint8) for p in (Y, Cb, Cr)]


def _events(stream, fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_times(args, emit):
    import torch
    import theora_amd
    from theora_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(1)
    s = torch.cuda.Stream()
    for size, (w, h) in SIZES.items():
        img = torch.from_numpy(rng.integers(0, 256, (h, w, 4), dtype=np.uint8)).cuda()
        for fmt in FORMATS:
            src = img if fmt == "rgba" else img[..., :3].contiguous() if fmt == "rgb" else img[..., :3].permute(2, 0, 1).contiguous()
            for pfname, pf in PIXEL_FMTS.items():
                outs = [torch.empty(sh, dtype=torch.uint8, device="cuda") for sh in theora_amd.picture_in_shapes(w, h, pf)]
                _, _, ptrs, pitches = theora_amd._pic_src(fmt, src)
                r = _lib.PictureInReq()
                r.format, r.pixel_fmt, r.width, r.height = theora_amd.PIC_FORMATS[fmt], pf, w, h
                for p in range(3):
                    r.src[p], r.src_pitch[p] = ptrs[p], pitches[p]
                    r.dst[p], r.dst_pitch[p] = outs[p].data_ptr(), outs[p].stride(0)
                h_s = s.cuda_stream
                with torch.cuda.stream(s):
                    for _ in range(20):
                        _lib.check(L.thip_picture_in(r, 1, h_s), "thip_picture_in")
                    want = torch_convert(src, fmt, pf)
                    s.synchronize()
                    if not all(torch.equal(a, b) for a, b in zip(outs, want)):
                        raise SystemExit("picture_in_time: the torch restatement and the kernel differ (%s %s %s)" % (size, fmt, pfname))
                    us = _events(s, lambda: L.thip_picture_in(r, 1, h_s), args.iters)
                    for _ in range(3):
                        torch_convert(src, fmt, pf)
                    t_us = _events(s, lambda: torch_convert(src, fmt, pf), max(args.iters // 10, 10))
                nbytes = floor_bytes(fmt, pf, w, h)
                fl = nbytes / BANDWIDTH * 1e6
                emit(dict(kind="kernel", size=size, format=fmt, pixel_fmt=pfname, iters=args.iters, us_per_launch=round(us, 2),
                          floor_bytes=nbytes, floor_us=round(fl, 2), times_floor=round(us / fl, 2), TB_s=round(nbytes / us / 1e6, 3),
                          torch_ops_us=round(t_us, 1), torch_over_kernel=round(t_us / us, 1)))


def encode_times(args, emit):
    """1080p, quality 48, device packetiser on: the time of one input call + packetout, R'G'B' tensors against Y'CbCr tensors."""
    import torch
    import theora_amd
    from theora_amd.encoder import Encoder
    w, h = 1920, 1080
    rng = np.random.default_rng(2)
    y, x = np.mgrid[0:h, 0:w]
    frames = []
    for f in range(8):
        base = np.stack([(x + 3 * f + y // 2) % 256, (2 * x + y + 5 * f) % 256, (x // 3 + 2 * y) % 256], -1)
        frames.append(torch.from_numpy(np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8)).cuda())
    planes = [theora_amd.picture_in([fr], 0, "rgb")[0] for fr in frames]
    torch.cuda.synchronize()
    for inter in (False, True):
        for kind in ("rgb", "ycbcr"):
            e = Encoder(1920, 1088, 0, 48, pic=(0, 0, w, h), inter=inter, device_pack=True)
            e.header_packets()
            times, nbytes = [], 0
            for n in range(args.enc_frames + 8):
                t0 = time.perf_counter()
                if kind == "rgb":
                    e.encode_rgb(frames[n % 8])
                else:
                    e.encode(planes[n % 8])
                pkt = e.packetout(False)
                dt = time.perf_counter() - t0
                if n >= 8:       # (the first frames allocate)
                    times.append(dt)
                    nbytes += len(pkt[0])
            e.close()
            emit(dict(kind="encode", size="1080p", quality=48, inter=inter, input=kind, frames=len(times),
                      median_ms=round(1e3 * statistics.median(times), 3), mean_ms=round(1e3 * statistics.fmean(times), 3),
                      bytes_per_frame=nbytes // len(times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--enc-frames", type=int, default=48)
    ap.add_argument("--jsonl", default=None, help="append the raw lines to this file")
    ap.add_argument("--skip-enc", action="store_true", help="kernel timings only")
    args = ap.parse_args()
    if args.iters < 100:
        raise SystemExit("picture_in_time: at least 100 launches a measurement")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("picture_in_time: no GPU (the numbers are device times; there is nothing to measure here)")
    out = open(args.jsonl, "a") if args.jsonl else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    kernel_times(args, emit)
    if not args.skip_enc:
        encode_times(args, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
