"""Drift-aware alignment on 256 clips x 10 s (8 distinct pairs with known lines, repeated 32 times): the wall time of
Engine-level align_drift (nhans_align at max_lag 800, two tracking passes, the host fits) and of one warp call, the
per-launch times of five more of each (nhans_profile_json) with the float64 rate of drift_track and the fused
multiply-add rate and bytes per second of drift_warp, nhans_align at max_lag 800 in the same run as the same-machine
basis, whether the lines are the planted ones and the results repeat with the clips bit for bit.  What
profiles/drift/README.md reports.
    python tools/drift_measure.py [--json out.json]"""
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
args = ap.parse_args()

NC, N, D, TRACK = 256, 160000, 800, 64
LINES = ((0.0, 0.0), (37.3, 50e-6), (-20.75, -200e-6), (3.25, 500e-6), (11.6, 150e-6), (-140.5, 30e-6), (211.0, -80e-6), (0.4, 900e-6))
rng = np.random.default_rng(1)
f = rng.uniform(80.0, 5000.0, 120)
amp, ph = rng.uniform(0.2, 1.0, 120) / np.sqrt(f / 80.0), rng.uniform(0, 2 * np.pi, 120)


def signal(x):
    s = np.zeros(len(x))
    for k in range(0, len(f), 20):
        s += (amp[k:k + 20, None] * np.sin(2 * np.pi * f[k:k + 20, None] / 16000.0 * x[None, :] + ph[k:k + 20, None])).sum(axis=0)
    return 0.03 * (0.6 + 0.4 * np.sin(2 * np.pi * 0.9 / 16000.0 * x)) * s


base = []
t = signal(np.arange(N, dtype=np.float64))
for a, b in LINES:
    e = signal((np.arange(N, dtype=np.float64) - a) / (1.0 + b))
    e = e + rng.standard_normal(N) * np.sqrt(np.mean(e * e) * 1e-3)             # 30 dB
    base.append((e.astype(np.float32), t.astype(np.float32)))
sig = [torch.from_numpy(np.concatenate([base[i % 8][k] for i in range(NC)])).cuda() for k in range(2)]
off = [i * N for i in range(NC + 1)]
eng = engine.Engine("denoiser", None)
out = {"clips": NC, "samples": N, "max_lag": D, "track_lag": TRACK, "lines": [list(l) for l in LINES]}


def fit_all(rec, soff):
    rec = rec.cpu().numpy()
    return [hip.drift_fit(rec[soff[i]:soff[i + 1]], score.DRIFT_RHO_MIN, score.DRIFT_TRIM) for i in range(NC)]


def align_drift():
    """Context.align_drift on tensors that are already in HBM -> (lines, seconds on the host's fits)"""
    coarse = eng.align_device(sig[0], off, sig[1], off, max_lag=D).cpu().numpy()
    rec, soff = eng.drift_track_device(sig[0], off, sig[1], off, [(float(r[3]), 0.0) for r in coarse], radius=TRACK)
    t0 = time.time()
    fits = fit_all(rec, soff)
    host = time.time() - t0
    rec, soff = eng.drift_track_device(sig[0], off, sig[1], off, [(f["a"], f["b"]) if f["fit_ok"] else (float(r[3]), 0.0)
                                                                   for f, r in zip(fits, coarse)], radius=8)
    t0 = time.time()
    fits = fit_all(rec, soff)
    return fits, host + time.time() - t0


t0 = time.time(); fits, _ = align_drift(); torch.cuda.synchronize(); out["first_call_s"] = time.time() - t0
align_drift(); torch.cuda.synchronize()
walls, hosts = [], []
for _ in range(5):
    t0 = time.time(); fits, h = align_drift(); torch.cuda.synchronize(); walls.append(time.time() - t0); hosts.append(h)
out["align_drift_wall_s"], out["align_drift_host_fit_s"] = walls, hosts
out["fit_ok"] = [f["fit_ok"] for f in fits[:8]]
out["lines_found"] = [[f["a"], f["b"]] for f in fits[:8]]
out["segments_used"] = [f["n_used"] for f in fits[:8]]
out["all_equal_mod8"] = bool(all(fits[i] == fits[i % 8] or (not fits[i]["fit_ok"] and not fits[i % 8]["fit_ok"]) for i in range(NC)))
lines = [(f["a"], f["b"]) if f["fit_ok"] else (0.0, 0.0) for f in fits]
warp = lambda: eng.drift_warp_device(sig[0], off, off, lines)
y, yoff, rngs = warp(); torch.cuda.synchronize()
walls = []
for _ in range(5):
    t0 = time.time(); y, yoff, rngs = warp(); torch.cuda.synchronize(); walls.append(time.time() - t0)
out["warp_wall_s"], out["warp_samples"] = walls, int(yoff[-1])
yh = y.cpu().numpy()
out["warp_equal_mod8"] = bool(all(np.array_equal(yh[yoff[i]:yoff[i + 1]].view(np.uint32), yh[yoff[i % 8]:yoff[i % 8 + 1]].view(np.uint32))
                                  for i in range(8, NC)))
sdr = []
for i in range(8):
    w, (lo, hi) = yh[yoff[i]:yoff[i + 1]].astype(np.float64), rngs[i]
    tt = base[i][1][lo:hi].astype(np.float64)
    al = np.dot(w, tt) / np.dot(tt, tt)
    sdr.append(float(10 * np.log10(np.dot(al * tt, al * tt) / np.dot(w - al * tt, w - al * tt))))
out["warped_si_sdr_db"] = sdr
eng.set_option("profile", 1)
align_drift(); warp(); torch.cuda.synchronize()
hip.check(eng.lib.nhans_profile_reset(eng.handle))
REP = 5
for _ in range(REP):
    align_drift()
    warp()
torch.cuda.synchronize()
prof = hip.profile_dict(eng.handle)
eng.set_option("profile", 0)
out["profile_repeats"], out["profile"] = REP, prof
k = prof["drift_track"]
out["drift_track_tflops"] = k["flops"] / (k["ms"] * 1e-3) / 1e12
k = prof["drift_warp"]
out["drift_warp_gfma_per_s"] = 0.5 * k["flops"] / (k["ms"] * 1e-3) / 1e9
out["drift_warp_gbytes_per_s"] = k["bytes"] / (k["ms"] * 1e-3) / 1e9
out["drift_warp_fma_per_call"] = 0.5 * k["flops"] / REP
if args.json:
    with open(args.json, "w") as fjson:
        json.dump(out, fjson, indent=1)
print(json.dumps(out, indent=1))
eng.close()
