"""nhans_quality on 256 clips x 10 s (8 distinct pairs, repeated 32 times): the wall time of five calls after two warm-up
calls, the per-launch times of five more (nhans_profile_json) with each launch's share and float64 rate, the workspace
the plan takes, whether the records repeat with the clips bit for bit; nhans_stoi on the same batch on the same box; the
figures of the reference's demo pairs; and the host definition's time for one clip.  What profiles/quality/README.md
reports.
    python tools/quality_measure.py [--json out.json] [--no-host]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nhans_amd  # noqa: E402,F401
from nhans_amd import engine, hip, score  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None, help="also write the result there")
ap.add_argument("--no-host", action="store_true", help="skip the host definition's time (about ten seconds)")
args = ap.parse_args()

rng = np.random.default_rng(1)
NC, N = 256, 160000
base = []
for k in range(8):
    t = np.convolve(0.1 * rng.standard_normal(N + 8), [1.0, 0.9, 0.5, 0.2], mode="same")[:N] + 0.002 * rng.standard_normal(N)
    e = t + (0.01 + 0.01 * k) * rng.standard_normal(N)
    base.append((e.astype(np.float32), t.astype(np.float32)))
sig = [torch.from_numpy(np.concatenate([base[i % 8][k] for i in range(NC)])).cuda() for k in range(2)]
off = [i * N for i in range(NC + 1)]
eng = engine.Engine("denoiser", None)
frames = NC * score.quality_num_frames(N)
out = {"clips": NC, "samples": N, "frames": frames}


def timed(run, names):
    res = {}
    t0 = time.time(); r = run(); torch.cuda.synchronize(); res["first_call_s"] = time.time() - t0
    run(); torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.time(); r = run(); torch.cuda.synchronize(); walls.append(time.time() - t0)
    res["wall_s"] = walls
    eng.set_option("profile", 1)
    run(); torch.cuda.synchronize()
    hip.check(eng.lib.nhans_profile_reset(eng.handle))
    REP = 5
    for _ in range(REP):
        run()
    torch.cuda.synchronize()
    prof = hip.profile_dict(eng.handle)
    eng.set_option("profile", 0)
    res["profile_repeats"] = REP
    res["profile"] = {k: prof[k] for k in prof if k.startswith(names)}
    total = sum(v["ms"] for v in res["profile"].values())
    res["ms_per_call"] = {k: v["ms"] / REP for k, v in res["profile"].items()}
    res["share"] = {k: v["ms"] / total for k, v in res["profile"].items()}
    res["tflops"] = {k: v["flops"] / (v["ms"] * 1e-3) / 1e12 for k, v in res["profile"].items() if v["ms"] > 0}
    res["gbytes_per_s"] = {k: v["bytes"] / (v["ms"] * 1e-3) / 1e9 for k, v in res["profile"].items() if v["ms"] > 0}
    return r, res


r, res = timed(lambda: eng.quality_device(sig[0], off, sig[1], off), "quality")
rec = r.cpu().numpy()
res["workspace_plan_bytes"] = sum(256 * ((b + 255) // 256) for b in (NC * 56, 8 * (480 + 1024), 8 * 25 * 257, 4 * 2 * 25, 24 * frames))
res["all_equal_mod8"] = bool(all((rec[i].view(np.uint64) == rec[i % 8].view(np.uint64)).all() for i in range(NC)))
res["records_head"] = [score.quality_record(rec[i]) for i in range(8)]
out["quality"] = res
# STOI of the same batch on the same box (16 kHz: its conversion to 10 kHz included, as Context.stoi runs it)
_, res = timed(lambda: eng.stoi_device(sig[0], off, sig[1], off), "stoi")
out["stoi"] = res
g = np.load(os.path.join(ROOT, "tests", "golden", "score_demo_pairs.npz"))
demo = {}
for ex in ("example2", "example3"):
    s = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
    got = eng.quality([s["denoised"], s["mixed"]], [s["target"], s["target"]])
    demo[ex] = {"denoised": got[0], "mixed": got[1], "improvement": score.improvement(got[1], got[0])}
out["demo_pairs"] = demo
if not args.no_host:
    t0 = time.time()
    ref = score.quality_reference(base[1][0], base[1][1])
    out["host_reference_one_clip_s"] = time.time() - t0
    out["host_reference_llr"] = ref["llr"]
    out["device_llr_same_clip"] = float(rec[1, 4])
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
eng.close()
