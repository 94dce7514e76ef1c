"""Cost of the MVDR stage on the device: a batch of `--clips` clips of `--seconds` s at C = 4 and C = 8 through nhans_mvdr,
per launch (option "profile"), beside nhans_stft_features over the same channel-clips.  Prints one JSON object; what was
measured with it is in profiles/mvdr/README.md.

    python tools/mvdr_measure.py [--clips 256] [--seconds 10] [--reps 5] > profiles/mvdr/mvdr_measure.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine, spec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--clips", type=int, default=256)
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    eng = engine.Engine("denoiser")
    T = int(a.seconds * 16000 - spec.WIN) // spec.HOP + 1
    n = spec.WIN + spec.HOP * (T - 1)
    out = {"clips": a.clips, "frames_per_clip": T, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device="cuda").manual_seed(1)
    for C in (4, 8):
        planes = 0.1 * torch.randn(a.clips * C * n, device="cuda", generator=g)
        mask = torch.rand((a.clips * T, spec.BINS), device="cuda", generator=g)
        off = [i * n for i in range(a.clips + 1)]
        coff = [i * n for i in range(a.clips * C + 1)]
        eng.mvdr_device(planes, off, C, mask)               # warm: the workspace grows once
        eng.stft_features(planes, coff)
        eng.set_option("profile", 1)
        eng.profile_reset()
        for _ in range(a.reps):
            eng.mvdr_device(planes, off, C, mask)
            eng.stft_features(planes, coff)
        torch.cuda.synchronize()
        prof = eng.profile()
        eng.set_option("profile", 0)
        out["C=%d" % C] = prof
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
