"""nhans_bss_eval on 256 clips x 10 s at J = 2, L = 512 (8 distinct AR(1) triples repeated): the wall time of five calls
after two warm-up calls, the per-launch times of five more (nhans_profile_json), how far the device's free memory fell at
the first call, and whether the records repeat with the clips, bit for bit.  What profiles/bsseval/README.md reports.
    python tools/bss_measure.py [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from scipy.signal import lfilter
import nhans_amd  # noqa: E402,F401
from nhans_amd import engine, hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None, help="also write the result there")
args = ap.parse_args()

rng = np.random.default_rng(1)
def ar(n, a):
    return (0.1 * np.sqrt(1 - a * a) * lfilter([1.0], [1.0, -a], rng.standard_normal(n))).astype(np.float32)

NC, N, L = 256, 160000, 512
base = []
for i in range(8):
    s0, s1 = ar(N, 0.9), ar(N, 0.99)
    e = (0.8 * s0 + 0.2 * s1 + 0.005 * rng.standard_normal(N)).astype(np.float32)
    base.append((e, s0, s1))
sig = [torch.from_numpy(np.concatenate([base[i % 8][k] for i in range(NC)])).cuda() for k in range(3)]
off = [i * N for i in range(NC + 1)]
eng = engine.Engine("denoiser", None)
free0 = torch.cuda.mem_get_info()[0]
run = lambda: eng.bss_eval_device(sig[0], off, [(sig[1], off), (sig[2], off)], filt_len=L)
out = {}
t = time.time(); r = run(); torch.cuda.synchronize(); out["first_call_s"] = time.time() - t
out["workspace_growth_bytes"] = free0 - torch.cuda.mem_get_info()[0]
run(); torch.cuda.synchronize()
walls = []
for _ in range(5):
    t = time.time(); r = run(); torch.cuda.synchronize(); walls.append(time.time() - t)
out["wall_s"] = walls
eng.set_option("profile", 1)
run(); torch.cuda.synchronize()
hip.check(eng.lib.nhans_profile_reset(eng.handle))
REP = 5
for _ in range(REP):
    run()
torch.cuda.synchronize()
prof = hip.profile_dict(eng.handle)
out["profile_repeats"] = REP
out["profile"] = prof
rec = r.cpu().numpy()
out["records_head"] = rec[:2].tolist()
out["all_equal_mod8"] = bool(all((rec[i].view(np.uint64) == rec[i % 8].view(np.uint64)).all() for i in range(NC)))
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
eng.close()
