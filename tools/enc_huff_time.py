"""Trained Huffman codes against the built-in ones (include/theoraenc_hip.h, "Huffman codes"), 1080p 4:2:0, the panning sequence of
tests/enc_inter_ref.py: bytes, and the quality statistics where a code set changes decisions.

  python tools/enc_huff_time.py [--frames 12] [--json out.jsonl]
      per setting -- key-only at quality 24 / 40 / 56; eight-mode inter frames; the full rate-distortion stack (block qi 8, masking
      4, RD modes, skip, level choice 3) at quality 36 / 40 / 44; bitrate mode -- one pass with the built-in codes (the parent's
      bytes: without the new calls every packet is the parent's), then a pass with codes trained on that pass's histograms (`self`),
      and a pass with codes trained on its first half (`half`: its bytes over the second half are against the built-in pass's second
      half).  One JSON line a pass.
  python tools/enc_huff_time.py --times [--frames 40] [--json out.jsonl]
      the device stage with the device packetiser on: per frame TH_ENCCTL_THIP_GET_TIMES' device time and the packetiser's own
      (TH_ENCCTL_THIP_GET_PACK_STATS), median and the 10th / 90th percentile.  Uses nothing newer than the device packetiser, so the
      same script runs on an older checkout (PYTHONPATH) for an A/B in one session.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)   # (behind PYTHONPATH: an older checkout's package may stand in front)
W, H, PIC = 1920, 1088, (0, 0, 1920, 1080)

RD = dict(all_modes=True, block_qi=8, masking=4, rd_modes=True, rd_skip=True, rd_quant=3)
SETTINGS = [("key-only", q, dict()) for q in (24, 40, 56)] + [("eight-modes", 40, dict(inter=True, all_modes=True))] + \
           [("rd-stack", q, dict(inter=True, **RD)) for q in (36, 40, 44)] + \
           [("bitrate-6M", 32, dict(inter=True, all_modes=True, bitrate=6000000))]


def one_pass(frames, q, codes, kw):
    """-> per packet (bytes, histogram, qi, ssim_q20 luma, sse luma)."""
    from theora_amd.encoder import Encoder
    e = Encoder(W, H, 0, q, pic=PIC, device_pack=True, huffman=codes, **kw)
    e.set_quality_stats(("sse", "ssim"))
    e.header_packets()
    out = []
    for f, fr in enumerate(frames):
        e.encode(fr)
        while True:
            r = e.packetout(f == len(frames) - 1)
            if r is None:
                break
            qs = e.quality_stats()
            out.append((len(r[0]), e.token_hist(), e.stats()["qi"], qs["ssim_q20"][0] / max(qs["windows"][0], 1) / float(1 << 20), qs["sse"][0]))
    e.close()
    return out


def summary(rows, lo=0):
    rows = rows[lo:]
    return dict(bytes=sum(r[0] for r in rows), ssim_y=round(float(np.mean([r[3] for r in rows])), 6),
                sse_y=int(sum(r[4] for r in rows)), qi_mean=round(float(np.mean([r[2] for r in rows])), 2), packets=len(rows))


def compare(frames, emit):
    from theora_amd.encoder import train_huffman
    n = len(frames)
    for name, q, kw in SETTINGS:
        base = one_pass(frames, q, None, kw)
        emit(dict(setting=name, quality=q, codes="built-in", frames=n, **summary(base), second_half=summary(base, n // 2)))
        for how, pool in (("self", base), ("half", base[:n // 2])):
            codes, st = train_huffman([r[1] for r in pool])
            got = one_pass(frames, q, codes, kw)
            emit(dict(setting=name, quality=q, codes="trained-" + how, frames=n, train=st, **summary(got), second_half=summary(got, n // 2)))


def times(frames, nframes, emit):
    from theora_amd.encoder import Encoder
    for name, kw in (("key-only", dict()), ("eight-modes", dict(inter=True, all_modes=True))):
        e = Encoder(W, H, 0, 40, pic=PIC, device_pack=True, **kw)
        e.header_packets()
        dev, pack, call, nbytes = [], [], [], []
        for f in range(nframes + 4):
            t0 = time.perf_counter()
            e.encode(frames[f % len(frames)])
            r = e.packetout(f == nframes + 3)
            t1 = time.perf_counter()
            if f >= 4 and r[0]:   # (four frames of warm-up)
                dev.append(e.times()[0])
                pack.append(e.pack_stats()["pack_ms"])
                call.append((t1 - t0) * 1e3)
                nbytes.append(len(r[0]))
        e.close()
        pct = lambda v: [round(float(np.percentile(v, p)), 4) for p in (50, 10, 90)]
        emit(dict(setting=name, quality=40, lib=os.environ.get("AB_NAME", "this"), frames=len(dev), device_ms=pct(dev), pack_ms=pct(pack),
                  stage_ms=pct(np.add(dev, pack)), call_ms=pct(call), bytes=int(np.mean(nbytes))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--times", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    from tests import enc_inter_ref as R
    frames = R.sequence("pan", W, H, 0, 8 if a.times else (a.frames or 12), seed=1)
    frames = [[fr[0][:1080], fr[1][:540], fr[2][:540]] for fr in frames]
    out = open(a.json, "a") if a.json else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if a.times:
        times(frames, a.frames or 40, emit)
    else:
        compare(frames, emit)


if __name__ == "__main__":
    main()
