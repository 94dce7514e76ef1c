"""nhans_align on 256 clips x 10 s (8 distinct pairs with known delays, repeated 32 times) at max_lag 800 and 8000: the wall
time of five calls after two warm-up calls, the per-launch times of five more (nhans_profile_json) with the float64 rate
of align_corr, the workspace the plan takes, whether the delays are the planted ones and the records repeat with the
clips bit for bit; nhans_align_cut on the same batch; and the host definition's time for one clip at max_lag 800.  What
profiles/align/README.md reports.
    python tools/align_measure.py [--json out.json] [--no-host]"""
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
ap.add_argument("--no-host", action="store_true", help="skip the host definition's time (about half a minute)")
args = ap.parse_args()

rng = np.random.default_rng(1)
NC, N = 256, 160000
DELAYS = (0, 37, -123, 640, -777, 5000, -7999, 211)
base = []
for d in DELAYS:
    p = max(d, 0)
    s = 0.1 * rng.standard_normal(p + N + abs(d) + 1)
    t = s[p:p + N]
    e = s[p - d:p - d + N] + 0.05 * rng.standard_normal(N)
    base.append((e.astype(np.float32), t.astype(np.float32)))
sig = [torch.from_numpy(np.concatenate([base[i % 8][k] for i in range(NC)])).cuda() for k in range(2)]
off = [i * N for i in range(NC + 1)]
eng = engine.Engine("denoiser", None)
out = {"clips": NC, "samples": N, "delays": list(DELAYS)}
for D in (800, 8000):
    res = {}
    free0 = torch.cuda.mem_get_info()[0]
    run = lambda: eng.align_device(sig[0], off, sig[1], off, max_lag=D)
    t0 = time.time(); r = run(); torch.cuda.synchronize(); res["first_call_s"] = time.time() - t0
    res["workspace_growth_bytes"] = free0 - torch.cuda.mem_get_info()[0]
    res["workspace_plan_bytes"] = 256 * ((NC * 32 + 255) // 256) + 256 * ((NC * (2 * D + 1) * 8 + 255) // 256)
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
    res["profile"] = prof
    k = prof["align_corr"]
    res["align_corr_tflops"] = k["flops"] / (k["ms"] * 1e-3) / 1e12
    rec = r.cpu().numpy()
    want = [d if abs(d) <= D else None for d in DELAYS]
    res["delays_found"] = [int(v) for v in rec[:8, 3]]
    res["delays_as_planted"] = bool(all(w is None or int(rec[i, 3]) == w for i, w in enumerate(want)))
    res["rho_head"] = rec[:8, 5].tolist()
    res["all_equal_mod8"] = bool(all((rec[i].view(np.uint64) == rec[i % 8].view(np.uint64)).all() for i in range(NC)))
    out["D%d" % D] = res
# the cut of the same batch by the delays of the last call
delays = [int(v) for v in rec[:, 3]]
cut = lambda: eng.align_cut_device(sig[0], off, sig[1], off, delays)
cut(); torch.cuda.synchronize()
walls = []
for _ in range(5):
    t0 = time.time(); c = cut(); torch.cuda.synchronize(); walls.append(time.time() - t0)
out["cut_wall_s"] = walls
out["cut_samples"] = int(c[2][-1])
if not args.no_host:
    t0 = time.time()
    ref = score.align_reference(base[1][0], base[1][1], 800)
    out["host_reference_D800_one_clip_s"] = time.time() - t0
    out["host_reference_delay"] = ref["delay"]
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
eng.close()
