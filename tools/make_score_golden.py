#!/usr/bin/env python3
"""Writes tests/golden/score_demo_pairs.npz: the mixed / denoised / target triples the reference ships with its trained
denoiser's demo (DEMO_N-HANS/denoising/example2 and example3 -- audio the reference's programs wrote, data), whole, as
float32, and their float64 scores: score.reference_all of `denoised` and of `mixed` against `target`.

    python tools/make_score_golden.py /path/to/N-HANS

The tests read the .npz only (tests/test_score_host.py checks that the stored scores reproduce)."""
import glob
import os
import sys

import numpy as np
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nhans_amd  # noqa: E402,F401
from nhans_amd import score  # noqa: E402

EXAMPLES = ("example2", "example3")
SIGNALS = ("mixed", "denoised", "target")
SCORE_KEYS = score.FIELDS + ("loss", "lsd_db")


def as_float32(path):
    rate, x = wavfile.read(path)
    assert rate == 16000 and x.ndim == 1, (path, rate, x.shape)
    if x.dtype == np.int16:
        return (x.astype(np.float64) / 32768.0).astype(np.float32)
    assert x.dtype == np.float32, (path, x.dtype)
    return x


def main(ref_root):
    out = {"score_keys": np.array(SCORE_KEYS)}
    for ex in EXAMPLES:
        sig = {}
        for k in SIGNALS:
            (path,) = glob.glob(os.path.join(ref_root, "DEMO_N-HANS", "denoising", ex, "*_%s.wav" % k))
            sig[k] = as_float32(path)
            out["%s_%s" % (ex, k)] = sig[k]
        for k in ("mixed", "denoised"):
            rec = score.reference_all(sig[k], sig["target"])
            out["%s_%s_scores" % (ex, k)] = np.array([rec[name] for name in SCORE_KEYS], dtype=np.float64)
            print(ex, k, len(sig[k]), {name: round(rec[name], 4) for name in score.FIGURES})
    dst = os.path.join(ROOT, "tests", "golden", "score_demo_pairs.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
