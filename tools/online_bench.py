"""Online enhancement (nhans_online_*): push wall time and real-time factor for S live streams per object and pushes of
H hops (H x 10 ms of audio per stream), f16x3, synthetic weights.  One JSON line per (S, H):
  push_ms_p50 / p99   host clock around push + device synchronise, after a warm-up of every shape
  kernel_ms_per_push  sum of the per-kernel hipEvent times of nhans_profile_json over a separate profiled pass
  realtime_factor     S x pushed audio seconds / p50 push time (streams one GPU keeps up with per ... of real time)
  latency_ms          the algorithmic latency range from the output contract (look-ahead + one window, +- one hop)
    python tools/online_bench.py [--streams 1,8,64,256] [--hops 1,4,16] [--pushes 60]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nhans_amd  # noqa: E402,F401
from nhans_amd import apply, engine, hip, online, spec, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,64,256")
    ap.add_argument("--hops", default="1,4,16")
    ap.add_argument("--pushes", type=int, default=60, help="timed pushes per shape (after 40 warm-up pushes)")
    a = ap.parse_args()
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    audio = apply.normalise(synth.mixture(1, 30.0))
    lat = online.latency_ms()
    for S in [int(s) for s in a.streams.split(",")]:
        for H in [int(h) for h in a.hops.split(",")]:
            n = H * spec.HOP
            enh = online.OnlineEnhancer(eng, [ca] * S, [cb] * S)
            pos = [0]

            def push():
                i = pos[0] % (len(audio) - n)
                pos[0] += n
                enh.push([audio[i:i + n]] * S)

            for _ in range(40):              # past the 17-frame look-ahead: every push then runs the whole path
                push()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.pushes):
                t0 = time.perf_counter()
                push()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            eng.set_option("profile", 1)
            eng.profile_reset()
            for _ in range(10):
                push()
            prof = eng.profile()
            eng.set_option("profile", 0)
            enh.close()
            kern = sum(v["ms"] for v in prof.values()) / 10
            p50, p99 = float(np.percentile(ts, 50)), float(np.percentile(ts, 99))
            print(json.dumps({"streams": S, "hops_per_push": H, "push_audio_ms": H * 10, "push_ms_p50": round(p50, 3),
                              "push_ms_p99": round(p99, 3), "kernel_ms_per_push": round(kern, 3),
                              "launches_per_push": sum(v["calls"] for v in prof.values()) / 10,
                              "realtime_factor": round(S * H * 0.010 / (p50 / 1e3), 2),
                              "latency_ms": [lat[0], lat[1]], "precision": "f16x3", "weights": "synthetic seed 7"}),
                  flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
