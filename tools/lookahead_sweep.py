"""What a shorter look-ahead changes in the output: RMS and SI-SDR of den_L against den_17 (the full-window output) for
L in {0, 1, 2, 4, 8, 17}, per clip, one JSON line per (clip, L).  den_L is Engine.enhance(..., lookahead=L): what a live
stream of look-ahead L emits for the same samples (include/nhans_hip.h: "lookahead").

ON THE SYNTHETIC WEIGHTS THESE NUMBERS SAY NOTHING ABOUT AUDIBLE QUALITY: a seeded random network has learnt no use for its
future rows, so its sensitivity to them is arbitrary.  The tool is for whoever has the trained bundle -- point
NHANS_MODEL_DIR at it and pass --weights checkpoint -- and even then it measures the distance from the L = 17 output, not
from clean speech.
    python tools/lookahead_sweep.py [--kind denoiser] [--weights synthetic] [--neg neg.wav --pos pos.wav] [mix.wav ...]
  (no files: three synthetic clips with their synthetic contexts)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nhans_amd  # noqa: E402,F401
from nhans_amd import apply, engine, spec, synth  # noqa: E402

LS = (0, 1, 2, 4, 8, 17)


def si_sdr_db(est, ref):
    ref64, est64 = ref.astype(np.float64), est.astype(np.float64)
    s = ref64 * (np.dot(est64, ref64) / max(np.dot(ref64, ref64), 1e-30))
    return 10.0 * np.log10(max(np.dot(s, s), 1e-30) / max(np.dot(est64 - s, est64 - s), 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--kind", default=spec.DENOISER, choices=[spec.DENOISER, spec.SEPARATOR])
    ap.add_argument("--weights", default="synthetic", choices=["synthetic", "checkpoint"])
    ap.add_argument("--pos", default=None)
    ap.add_argument("--neg", default=None)
    a = ap.parse_args()
    if a.files and not (a.pos and a.neg):
        ap.error("files need --pos and --neg conditioning recordings")
    apply.FLAGS.weights = a.weights
    eng = engine.Engine(a.kind, apply._load_weights(a.kind) if a.weights == "checkpoint" else None, precision="f16x3")
    if a.files:
        apply.FLAGS.convert = True
        clips = []
        for f in a.files:
            pos_neg = (a.pos, a.neg) if a.kind == spec.DENOISER else (a.neg, a.pos)
            ca, cb, mix = apply.handle_signals(f, pos_neg[0], pos_neg[1], a.kind)
            clips.append((os.path.basename(f), mix, ca, cb))
    else:
        clips = [("synthetic %d" % i, apply.trim_to_frames(apply.normalise(synth.mixture(i, 3.0))),
                  apply.normalise(synth.silent()), apply.normalise(synth.noise_context(i))) for i in (1, 2, 3)]
    for name, mix, ca, cb in clips:
        ref = eng.enhance([mix], [ca], [cb], want_mixed=False)["denoised_wav"][0]
        for L in LS:
            den = eng.enhance([mix], [ca], [cb], want_mixed=False, lookahead=L)["denoised_wav"][0]
            diff = den.astype(np.float64) - ref
            print(json.dumps({"clip": name, "lookahead": L, "latency_ms": [10 * L + 15, 10 * L + 35],
                              "rms_vs_den17": float(np.sqrt(np.mean(diff * diff))),
                              "rms_den17": float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))),
                              "si_sdr_db_vs_den17": None if L == 17 else round(si_sdr_db(den, ref), 2),
                              "weights": a.weights, "kind": a.kind}), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
