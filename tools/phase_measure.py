"""Phase refinement on 256 clips x 10 s (8 distinct synthetic mixtures, repeated 32 times; 998 frames each): the wall time of
nhans_phase_refine at N = 8 and N = 32 (with and without the inconsistencies, with and without momentum) against the same
number of nhans_istft + nhans_stft_features call pairs on the same rows in the same process, the per-launch times of both
(nhans_profile_json), whether the results repeat with the clips bit for bit, and the time of one enhance step at
phase_iters = 0, 8 and 32.  What profiles/phase/README.md reports.
    python tools/phase_measure.py [--json out.json] [--no-enhance]"""
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
from nhans_amd import engine, hip, spec, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None, help="also write the result there")
ap.add_argument("--no-enhance", action="store_true", help="skip the enhance steps (5 s each)")
args = ap.parse_args()

NC, N = 256, 160000
f32 = lambda x: x.astype(np.float32) / np.float32(32768.0)
base = [f32(synth.mixture(i))[:N] for i in range(8)]
base = [b[:spec.WIN + spec.HOP * ((len(b) - spec.WIN) // spec.HOP)] for b in base]
n = len(base[0])
wav = torch.from_numpy(np.concatenate([base[i % 8] for i in range(NC)])).cuda()
off = [i * n for i in range(NC + 1)]
eng = engine.Engine("denoiser", None)
lm, ph = eng.stft_features(wav, off)
T = lm.shape[0] // NC
foff = [i * T for i in range(NC + 1)]
out = {"clips": NC, "frames_per_clip": T, "run": hip.PHASE_RUN}
sync = lambda: torch.cuda.synchronize()


def timed(fn, warm=2, rep=5):
    for _ in range(warm):
        fn()
    sync()
    w = []
    for _ in range(rep):
        t0 = time.time(); fn(); sync(); w.append(time.time() - t0)
    return w


def pairs(k):
    """k times: the waveform to HBM (nhans_istft) and back to rows (nhans_stft_features)"""
    a, b = lm, ph
    for _ in range(k):
        w, ooff = eng.istft(a, b, foff)
        a, b = eng.stft_features(w, ooff)


for k in (8, 32):
    out["refine_N%d_wall_s" % k] = timed(lambda: eng.phase_refine_rows(lm, ph, foff, k))
    out["refine_N%d_inc_wall_s" % k] = timed(lambda: eng.phase_refine_rows(lm, ph, foff, k, inc=True))
    out["refine_N%d_alpha_wall_s" % k] = timed(lambda: eng.phase_refine_rows(lm, ph, foff, k, 0.5))
    out["pairs_N%d_wall_s" % k] = timed(lambda: pairs(k))
r, inc = eng.phase_refine_rows(lm, ph, foff, 8, inc=True)
rh, ih = r.cpu().numpy().reshape(NC, T, spec.BINS), inc.cpu().numpy()
out["equal_mod8"] = bool(all(rh[i].tobytes() == rh[i % 8].tobytes() and ih[i].tobytes() == ih[i % 8].tobytes() for i in range(8, NC)))
out["inc_db_clip0"] = [float(10 * np.log10(v)) for v in ih[0]]
eng.set_option("profile", 1)
REP = 5
for name, fn in (("refine_N8", lambda: eng.phase_refine_rows(lm, ph, foff, 8)), ("refine_N8_inc", lambda: eng.phase_refine_rows(lm, ph, foff, 8, inc=True)),
                 ("refine_N8_alpha", lambda: eng.phase_refine_rows(lm, ph, foff, 8, 0.5)), ("pairs_N8", lambda: pairs(8))):
    fn(); sync()
    hip.check(eng.lib.nhans_profile_reset(eng.handle))
    for _ in range(REP):
        fn()
    sync()
    out["profile_" + name] = hip.profile_dict(eng.handle)
eng.set_option("profile", 0)
out["profile_repeats"] = REP
if not args.no_enhance:
    ctx = [f32(synth.noise_context(i)) for i in range(16)]
    ca, ca_off = eng._dev([ctx[i % 8] for i in range(NC)])
    cb, cb_off = eng._dev([ctx[8 + i % 8] for i in range(NC)])
    step = lambda: eng.enhance_device(wav, off, ca, ca_off, cb, cb_off)
    step(); sync()
    for k in (0, 8, 32):
        eng.set_option("phase_iters", k)
        step(); sync()
        t0 = time.time(); step(); sync(); out["enhance_step_N%d_s" % k] = time.time() - t0
    eng.set_option("phase_iters", 0)
if args.json:
    with open(args.json, "w") as fjson:
        json.dump(out, fjson, indent=1)
print(json.dumps(out, indent=1))
eng.close()
