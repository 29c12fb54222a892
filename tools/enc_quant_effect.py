#!/usr/bin/env python3
"""What a caller's quantisers change: the built-in quantisation parameters against those of the reference encoder, the latter parsed
from the setup header stored in tests/golden/ref_qcif_q32.npz (thip_quant_info_from_setup), on the 352 x 288 `pan` and `cut` clips of
tests/enc_inter_ref.py (`cut` is the pan that cuts to noise half way, the module's noise content), 10 frames, inter frames on, with and without the full rate-distortion stack.  Bytes, Y PSNR and SSIM per
quality from TH_ENCCTL_THIP_GET_QUALITY_STATS -> profiles/enc_quant_effect.json.  Reports what comes out; asserts nothing.
usage: python tools/enc_quant_effect.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import enc_inter_ref as R   # noqa: E402
from theora_amd import encoder as E   # noqa: E402

W, H, N = 352, 288, 10
QUALITIES = (16, 24, 32, 40, 48, 56)
STACKS = {"plain": dict(), "rd": dict(all_modes=True, block_qi=8, masking=4, rd_modes=True, rd_skip=True, rd_quant=True)}


def ref_quant():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_qcif_q32.npz"))
    n = [int(v) for v in g["lengths"][:3]]
    return E.quant_from_setup(g["data"][n[0] + n[1]:n[0] + n[1] + n[2]].tobytes())


def run(frames, q, quant, **kw):
    e = E.Encoder(W, H, 0, q, inter=True, keyframe_interval=64, quant=quant, **kw)
    e.set_quality_stats(("sse", "ssim"))
    e.header_packets()
    nbytes, sse, ssim = 0, 0, 0.0
    for f, fr in enumerate(frames):
        e.encode(fr)
        nbytes += len(e.packetout(f == len(frames) - 1)[0])
        st = e.quality_stats()
        sse += st["sse"][0]
        ssim += st["ssim"][0] or 0.0
    e.close()
    mse = sse / (len(frames) * W * H)
    return dict(bytes=nbytes, psnr_y=round(10 * np.log10(255 * 255 / max(mse, 1e-9)), 3), ssim_y=round(ssim / len(frames), 5))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "enc_quant_effect.json")
    quants = {"built-in": None, "reference": ref_quant()}
    rows = []
    for clip in ("pan", "cut"):
        frames = R.sequence(clip, W, H, 0, N, seed=1)
        for stack, kw in STACKS.items():
            for q in QUALITIES:
                for name, quant in quants.items():
                    rows.append(dict(clip=clip, stack=stack, quality=q, quantisers=name, **run(frames, q, quant, **kw)))
                    print(rows[-1], flush=True)
    with open(out, "w") as f:
        json.dump(dict(width=W, height=H, frames=N, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
