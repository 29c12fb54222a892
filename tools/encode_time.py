"""The intra encoder (th_encode_*) per frame: the device stage (HIP events around its four launches and read-backs,
TH_ENCCTL_THIP_GET_TIMES), the host's part of th_encode_packetout (EOB runs, tables, bits), packet bytes and Y/Cb/Cr PSNR of the
decoded picture (the encoder's own quality statistics, TH_ENCCTL_THIP_GET_QUALITY_STATS, from a run of their own) -- 720p, 1080p and 4K at 4:2:0, the seeded natural image of tests/enc_ref.py, quality 16 and 48.  Kernel times
come from a separate `rocprofv3 --kernel-trace --stats -- python tools/encode_time.py --frames 8` run.

With --inter N: inter frames with a key frame every N frames (TH_ENCCTL_THIP_SET_INTER_FRAMES) on the panning sequence of
tests/enc_inter_ref.py; device and host times are medians over the inter frames, bytes the mean packet, PSNR the mean of the decoded
frames.  call_ms includes the reconstruction (the encoder's own decoder) that sits between two frames.  With --all-modes as well,
each case runs with all eight macro-block modes off and then on (TH_ENCCTL_THIP_SET_INTER_MODES), in the same process.

With --bitrate B: bitrate mode at B bits a second (30 fps), key frames (intra-only) and inter frames (a key frame every --inter N,
default 12) of the panning sequence: per frame type the medians of the probe's device time (probe_ms), the controller (control_ms),
the frame's device stage after it (device_ms) and the whole call (call_ms), next to quality mode at the median qi chosen (q_*).

With --device-pack each case runs with the device packetiser off and then on (TH_ENCCTL_THIP_SET_DEVICE_PACK), in the same process;
pack_ms is the packetiser's own device time (TH_ENCCTL_THIP_GET_PACK_STATS), call_spread the (min, max) of the call times.

With --auto-keyframes [T] (with --inter or --bitrate) each case runs with automatic key frames off and then on at the ratio T
(TH_ENCCTL_THIP_SET_AUTO_KEYFRAMES; default 230), in the same process; measure_ms is the measurement's own device time
(TH_ENCCTL_THIP_GET_CUT_STATS: the search, the sums and the 32 bytes on the host), which device_ms does not include, and cut_frames
counts the key frames it made (none on the panning sequence).

With --masking K (with --block-qi, in quality mode): activity masking at ratio K (TH_ENCCTL_THIP_SET_MASKING); mask_ms is the device
time of its two launches (TH_ENCCTL_THIP_GET_MASK_STATS), which device_ms includes.

With --roi RES (with --block-qi, key frames in quality mode): a region-of-interest map (TH_ENCCTL_THIP_SET_ROI_MAP) at macro-block
resolution (RES = mb) or pixel resolution (RES = pixel), seeded noise in +-32 set once from host memory; roi_ms is the device time of
its two launches (TH_ENCCTL_THIP_GET_ROI_STATS), which device_ms includes.

With --rd-modes (with --inter N --all-modes): the eight-mode cases run with the rate-distortion mode decision on
(TH_ENCCTL_THIP_SET_RD_MODES); rd_ms is the device time of its two launches (TH_ENCCTL_THIP_GET_RD_STATS), which device_ms includes.
--rd-skip: with --inter, every case with the skip decision on (TH_ENCCTL_THIP_SET_RD_SKIP); skip_ms is the device time of its two
launches (TH_ENCCTL_THIP_GET_SKIP_STATS), which device_ms includes.
--rd-quant W: every case (key-only and --inter) with the level choice on at weight W (TH_ENCCTL_THIP_SET_RD_QUANT); rdq_ms is the
device time of its launch (TH_ENCCTL_THIP_GET_RD_QUANT_STATS), which device_ms includes, rdq_zeroed / rdq_lowered the levels it changed
a frame.
Switch off and on are two runs of the tool.

With --two-pass (with --bitrate B for the second pass's target, default 8 Mbit/s; --inter N as with --bitrate): per size and frame
type, quality mode at 32 without and with TH_ENCCTL_THIP_2PASS_OUT -- in_ms is the time inside th_encode_ycbcr_in alone (it never
waits in quality mode, first pass or not), call_ms the whole call with th_encode_packetout, p1_probe_ms the probe's device time and
p1_wait_ms the host's wait in th_encode_packetout for its 512 bytes (TH_ENCCTL_THIP_GET_2PASS_STATS) -- and then the second pass over
that pass file (p2_*; its probe is waited for, as in bitrate mode).

  python tools/encode_time.py [--two-pass] [--frames 20] [--inter N [--all-modes [--rd-modes]] [--rd-skip]] [--rd-quant W] [--bitrate B] [--block-qi D [--masking K] [--roi mb|pixel]] [--device-pack]
                              [--auto-keyframes [T]] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"720p": (1280, 720, None), "1080p": (1920, 1088, (0, 0, 1920, 1080)), "4k": (3840, 2160, None)}


def psnr(sse, samples):
    """From the encoder's quality statistics (TH_ENCCTL_THIP_GET_QUALITY_STATS): the exact sums the device made."""
    return 99.0 if sse == 0 else 10 * np.log10(255.0 ** 2 / (sse / samples))


def quality_pass(frames, *args, **kw):
    """The frames once more through an encoder of the same configuration with the quality statistics on -- a run of its own, so
    that the timed run above stays what it was; the switch changes no packet.  Returns per frame the statistics' dict."""
    from theora_amd.encoder import Encoder
    e = Encoder(*args, **kw)
    e.set_quality_stats("sse")
    e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        e.packetout(f == len(frames) - 1)
        out.append(e.quality_stats())
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--inter", type=int, default=0)
    ap.add_argument("--bitrate", type=int, default=0)
    ap.add_argument("--all-modes", action="store_true", help="with --inter: each case with all eight modes off, then on")
    ap.add_argument("--block-qi", type=int, default=0, help="block-level qi with this delta (TH_ENCCTL_THIP_SET_BLOCK_QI)")
    ap.add_argument("--masking", type=int, default=0, help="with --block-qi: activity masking at this ratio (TH_ENCCTL_THIP_SET_MASKING)")
    ap.add_argument("--roi", choices=("mb", "pixel"), help="with --block-qi, key frames: a region-of-interest map at this resolution")
    ap.add_argument("--rd-modes", action="store_true", help="with --inter --all-modes: the eight-mode cases with TH_ENCCTL_THIP_SET_RD_MODES on")
    ap.add_argument("--rd-skip", action="store_true", help="with --inter: every case with TH_ENCCTL_THIP_SET_RD_SKIP on")
    ap.add_argument("--rd-quant", type=int, default=0, metavar="W", help="every case with TH_ENCCTL_THIP_SET_RD_QUANT = W (1..64)")
    ap.add_argument("--device-pack", action="store_true", help="each case with the device packetiser off, then on")
    ap.add_argument("--auto-keyframes", type=int, nargs="?", const=230, default=0, metavar="T",
                    help="with --inter or --bitrate: each case with automatic key frames off, then on at ratio T (default 230)")
    ap.add_argument("--two-pass", action="store_true", help="quality mode without and with the first pass, then the second pass")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.two_pass:
        return main_two_pass(args)
    if args.bitrate:
        return main_bitrate(args)
    if args.inter:
        return main_inter(args)
    from tests import enc_ref
    from theora_amd.encoder import Encoder
    rows = []
    for name, (w, h, pic) in SIZES.items():
        p = pic or (0, 0, w, h)
        frame = enc_ref.picture("natural", w, h, 0, p, picture_size=True, seed=5)
        for q, dp in [(q, dp) for q in (16, 48) for dp in ((False, True) if args.device_pack else (False,))]:
            e = Encoder(w, h, 0, q, pic=pic, block_qi=args.block_qi, device_pack=dp, masking=args.masking, rd_quant=args.rd_quant)
            hdr = e.header_packets()
            dev, host, wall, pack, mask, zqms, roims = [], [], [], [], [], [], []
            if args.roi:
                mw, mh = (p[2], p[3]) if args.roi == "pixel" else ((p[2] + 15) // 16, (p[3] + 15) // 16)
                e.set_roi(np.random.default_rng(7).integers(-32, 33, (mh, mw)).astype(np.int8))
            for f in range(args.frames + 3):
                t0 = time.perf_counter()
                e.encode(frame)
                pkt = e.packetout()[0]
                t1 = time.perf_counter()
                d, hm = e.times()
                if f >= 3:
                    dev.append(d)
                    host.append(hm)
                    wall.append((t1 - t0) * 1e3)
                    pack.append(e.pack_stats()["pack_ms"])
                    mask.append(e.mask_stats()["mask_ms"])
                    zqms.append(e.rd_quant_stats()["rdq_ms"])
                    roims.append(e.roi_stats()["roi_ms"])
            st = e.stats()
            e.close()
            qs = quality_pass([frame], w, h, 0, q, pic=pic, block_qi=args.block_qi, device_pack=dp, masking=args.masking,
                              rd_quant=args.rd_quant)[0]
            ps = [round(psnr(qs["sse"][pl], qs["samples"][pl]), 2) for pl in range(3)]
            r = dict(size=name, quality=q, device_ms=round(float(np.median(dev)), 4), host_ms=round(float(np.median(host)), 4),
                     call_ms=round(float(np.median(wall)), 4), bytes=len(pkt), tokens=st["tokens"],
                     tokens_merged=st["tokens_merged"], psnr=ps)
            if args.device_pack:
                r.update(device_pack=dp, pack_ms=round(float(np.median(pack)), 4),
                         call_spread=[round(float(min(wall)), 4), round(float(max(wall)), 4)])
            if args.masking:
                r.update(masking=args.masking, mask_ms=round(float(np.median(mask)), 4))
            if args.rd_quant:
                r.update(rd_quant=args.rd_quant, rdq_ms=round(float(np.median(zqms)), 4))
            if args.roi:
                r.update(roi=args.roi, roi_ms=round(float(np.median(roims)), 4))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)


def main_inter(args):
    from tests import enc_inter_ref, enc_ref
    from theora_amd.encoder import Encoder
    rows = []
    n = args.frames + 3
    for name, (w, h, pic) in SIZES.items():
        p = pic or (0, 0, w, h)
        frames = [[a[:enc_ref.chroma_region(p, 0, k)[3], :enc_ref.chroma_region(p, 0, k)[2]] for k, a in enumerate(fr)]
                  for fr in enc_inter_ref.sequence("pan", w, h, 0, n, seed=5)]
        for q, am, dp, ak in [(q, am, dp, ak) for q in (16, 48) for am in ((False, True) if args.all_modes else (False,))
                              for dp in ((False, True) if args.device_pack else (False,))
                              for ak in ((0, args.auto_keyframes) if args.auto_keyframes else (0,))]:
            e = Encoder(w, h, 0, q, pic=pic, inter=True, keyframe_interval=args.inter, all_modes=am, block_qi=args.block_qi,
                        device_pack=dp, auto_keyframes=ak, masking=args.masking, rd_modes=args.rd_modes and am, rd_skip=args.rd_skip,
                        rd_quant=args.rd_quant)
            hdr = e.header_packets()
            dev, host, wall, pkts, keys, pack, meas, cuts, mask, rdms, skms, zqms, zq0, zq1 = [], [], [], [], 0, [], [], 0, [], [], [], [], [], []
            for f in range(n):
                t0 = time.perf_counter()
                e.encode(frames[f])
                pkt = e.packetout(f == n - 1)[0]
                t1 = time.perf_counter()
                d, hm = e.times()
                key = e.inter_stats()["key"]
                pkts.append(pkt)
                if f >= 3 and not key and pkt:
                    dev.append(d)
                    host.append(hm)
                    wall.append((t1 - t0) * 1e3)
                    pack.append(e.pack_stats()["pack_ms"])
                    meas.append(e.cut_stats()["measure_ms"])
                    mask.append(e.mask_stats()["mask_ms"])
                    rdms.append(e.rd_stats()["rd_ms"])
                    skms.append(e.skip_stats()["skip_ms"])
                    zq = e.rd_quant_stats()
                    zqms.append(zq["rdq_ms"])
                    zq0.append(sum(zq["zeroed"]))
                    zq1.append(sum(zq["lowered"]))
                keys += key
                cuts += e.cut_stats()["cut"]
            e.close()
            ps = [psnr(qs["sse"][0], qs["samples"][0])
                  for qs in quality_pass(frames, w, h, 0, q, pic=pic, inter=True, keyframe_interval=args.inter, all_modes=am,
                                         block_qi=args.block_qi, device_pack=dp, auto_keyframes=ak, masking=args.masking,
                                         rd_modes=args.rd_modes and am, rd_skip=args.rd_skip, rd_quant=args.rd_quant)]
            r = dict(size=name, quality=q, inter=args.inter, all_modes=am, key_frames=keys, device_ms=round(float(np.median(dev)), 4),
                     host_ms=round(float(np.median(host)), 4), call_ms=round(float(np.median(wall)), 4),
                     bytes=int(np.mean([len(x) for x in pkts])), psnr_y=round(float(np.mean(ps)), 2))
            if args.device_pack:
                r.update(device_pack=dp, pack_ms=round(float(np.median(pack)), 4),
                         call_spread=[round(float(min(wall)), 4), round(float(max(wall)), 4)])
            if args.auto_keyframes:
                r.update(auto_keyframes=ak, measure_ms=round(float(np.median(meas)), 4), cut_frames=cuts)
            if args.masking:
                r.update(masking=args.masking, mask_ms=round(float(np.median(mask)), 4))
            if args.rd_modes:
                r.update(rd_modes=bool(am), rd_ms=round(float(np.median(rdms)), 4))
            if args.rd_skip:
                r.update(rd_skip=True, skip_ms=round(float(np.median(skms)), 4))
            if args.rd_quant:
                r.update(rd_quant=args.rd_quant, rdq_ms=round(float(np.median(zqms)), 4), rdq_zeroed=int(np.mean(zq0)),
                         rdq_lowered=int(np.mean(zq1)))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)


def _timed(e, frames, keep):
    """Encodes frames; per frame kept by keep(stats dict): (call ms, device ms, rate stats or None, measure ms)."""
    out = []
    for f, fr in enumerate(frames):
        t0 = time.perf_counter()
        e.encode(fr)
        e.packetout(f == len(frames) - 1)
        t1 = time.perf_counter()
        st = e.rate_stats() if e.bitrate else None
        if f >= 3 and keep(e, st):
            out.append(((t1 - t0) * 1e3, e.times()[0], st, e.cut_stats()["measure_ms"]))
    return out


def main_bitrate(args):
    from tests import enc_inter_ref, enc_ref
    from theora_amd.encoder import Encoder
    rows = []
    n = args.frames + 3
    kf = args.inter or 12
    for name, (w, h, pic) in SIZES.items():
        p = pic or (0, 0, w, h)
        frames = [[a[:enc_ref.chroma_region(p, 0, k)[3], :enc_ref.chroma_region(p, 0, k)[2]] for k, a in enumerate(fr)]
                  for fr in enc_inter_ref.sequence("pan", w, h, 0, n, seed=5)]
        for kind, ak in [("key", 0), ("inter", 0)] + ([("inter", args.auto_keyframes)] if args.auto_keyframes else []):
            inter = kind == "inter"
            want_key = not inter

            def keep(e, st):
                return not st["dropped"] and not st["duplicate"] and bool(st["key"]) == want_key
            e = Encoder(w, h, 0, 32, pic=pic, inter=inter, keyframe_interval=kf if inter else None, bitrate=args.bitrate,
                        auto_keyframes=ak)
            e.header_packets()
            rr = _timed(e, frames, keep)
            e.close()
            qi = int(np.median([r[2]["qi"] for r in rr]))
            e = Encoder(w, h, 0, qi, pic=pic, inter=inter, keyframe_interval=kf if inter else None, auto_keyframes=ak)
            e.header_packets()
            qq = _timed(e, frames, lambda e, st: e.inter_stats()["key"] == want_key)
            e.close()
            med = lambda xs: round(float(np.median(xs)), 4)
            r = dict(size=name, frames=kind, bitrate=args.bitrate, qi=qi, n=len(rr), call_ms=med([x[0] for x in rr]),
                     probe_ms=med([x[2]["probe_ms"] for x in rr]), control_ms=med([x[2]["control_ms"] for x in rr]),
                     device_ms=med([x[1] for x in rr]), q_call_ms=med([x[0] for x in qq]), q_device_ms=med([x[1] for x in qq]))
            if args.auto_keyframes:
                r.update(auto_keyframes=ak, measure_ms=med([x[3] for x in rr]), q_measure_ms=med([x[3] for x in qq]))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)


def main_two_pass(args):
    from tests import enc_inter_ref, enc_ref
    from theora_amd.encoder import Encoder
    rows = []
    n = args.frames + 3
    kf = args.inter or 12
    bitrate = args.bitrate or 8000000
    med = lambda xs: round(float(np.median(xs)), 4)
    for name, (w, h, pic) in SIZES.items():
        p = pic or (0, 0, w, h)
        frames = [[a[:enc_ref.chroma_region(p, 0, k)[3], :enc_ref.chroma_region(p, 0, k)[2]] for k, a in enumerate(fr)]
                  for fr in enc_inter_ref.sequence("pan", w, h, 0, n, seed=5)]
        for kind in ("key", "inter"):
            inter = kind == "inter"
            kw = dict(pic=pic, inter=inter, keyframe_interval=kf if inter else None)

            def run(e, record, feed=None):
                """Per kept frame (in ms, call ms, device ms, two-pass stats); the pass file when recording."""
                e.header_packets()
                data = [e.two_pass_out()] if record else []
                if feed is not None:
                    assert e.two_pass_in(feed) == len(feed)
                out = []
                for f, fr in enumerate(frames):
                    t0 = time.perf_counter()
                    e.encode(fr)
                    t1 = time.perf_counter()
                    e.packetout(f == n - 1)
                    t2 = time.perf_counter()
                    tp = e.two_pass_stats()
                    if record:
                        data.append(e.two_pass_out())
                    if f >= 3 and bool(e.inter_stats()["key"]) == (not inter):
                        out.append(((t1 - t0) * 1e3, (t2 - t0) * 1e3, e.times()[0], tp))
                if record:
                    data[0] = e.two_pass_out()   # the finished header over the placeholder
                e.close()
                return out, b"".join(data)
            q0, _ = run(Encoder(w, h, 0, 32, **kw), False)
            q1, data = run(Encoder(w, h, 0, 32, **kw), True)
            p2, _ = run(Encoder(w, h, 0, 32, bitrate=bitrate, **kw), False, feed=data)
            r = dict(size=name, frames=kind, n=len(q1), q_in_ms=med([x[0] for x in q0]), q_call_ms=med([x[1] for x in q0]),
                     q_device_ms=med([x[2] for x in q0]), p1_in_ms=med([x[0] for x in q1]), p1_call_ms=med([x[1] for x in q1]),
                     p1_device_ms=med([x[2] for x in q1]), p1_probe_ms=med([x[3]["probe_ms"] for x in q1]),
                     p1_wait_ms=med([x[3]["wait_ms"] for x in q1]), p1_wait_max_ms=round(max(x[3]["wait_ms"] for x in q1), 4),
                     bitrate=bitrate, p2_qi=int(np.median([x[3]["qi"] for x in p2])), p2_in_ms=med([x[0] for x in p2]),
                     p2_call_ms=med([x[1] for x in p2]), p2_probe_ms=med([x[3]["probe_ms"] for x in p2]))
            print(json.dumps(r), flush=True)
            rows.append(r)
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
