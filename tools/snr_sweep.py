"""The denoiser over a directory of triples x a grid of SNR pairs x look-aheads, scored on the device in one pass per
look-ahead (apply.evaluate_corpus): a table of the mean si_sdr_i, snr_i, segsnr_i and loss_ratio of the denoised signal
over the mixture, per (snr_pos, snr_neg, look-ahead).  The recordings are read and uploaded once per look-ahead; mixing
(nhans_mix), STFT, tower, stack, iSTFT and scoring stay in HBM and only the records come back.

ON THE SYNTHETIC WEIGHTS THESE NUMBERS SAY NOTHING ABOUT QUALITY: a seeded random network denoises nothing.  The tool is
for whoever has the trained bundle -- point NHANS_MODEL_DIR at it and pass --weights checkpoint; with the synthetic
weights it shows that the plumbing runs.
    python tools/snr_sweep.py DIR [--snrs -3,0,3,5,8] [--lookaheads 17,8,2] [--weights synthetic] [--json out.json] [--stoi] [--bss] [--quality] [--phase_iters N]
  --stoi adds the columns stoi_i and estoi_i: STOI and extended STOI in the same pass (NaN for a job whose output is too
  short for one 30-frame segment: 4,097 samples at 10 kHz).
  --bss adds the columns sdr_i, sir_i and sar_i: BSS Eval against each job's own target and negative noise, in the same
  pass (filters of 512 taps).
  --quality adds the columns llr_i, cd_i and fwsegsnr_i: the log-likelihood ratio and the cepstral distance of the LPC
  models (LOWER is better: an improvement is negative) and the frequency-weighted segmental SNR, in the same pass.
  DIR holds <name>_speech.wav, <name>_pos.wav and <name>_neg.wav per triple (16 kHz int16; the speech longer than 200
  frames = 32,240 samples).  No DIR: three synthetic triples written to a temporary directory."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nhans_amd  # noqa: E402,F401
from nhans_amd import apply, engine, spec, synth  # noqa: E402

FIGURES = ("si_sdr_i", "snr_i", "segsnr_i", "loss_ratio")
STOI_FIGURES = ("stoi_i", "estoi_i")
BSS_FIGURES = ("sdr_i", "sir_i", "sar_i")
QUALITY_FIGURES = ("llr_i", "cd_i", "fwsegsnr_i")


def find_triples(directory):
    names = sorted(f[:-len("_speech.wav")] for f in os.listdir(directory) if f.endswith("_speech.wav"))
    triples = [tuple(os.path.join(directory, "%s_%s.wav" % (n, k)) for k in ("speech", "pos", "neg")) for n in names]
    missing = [p for t in triples for p in t if not os.path.isfile(p)]
    if missing:
        raise SystemExit("missing: " + ", ".join(missing))
    return triples


def synthetic_triples(directory):
    from scipy.io import wavfile
    for i in (1, 2, 3):
        for k, x in (("speech", synth.mixture(i, 3.0)), ("pos", synth.noise_context(i, 1.0)), ("neg", synth.speaker_context(i, 3.0))):
            wavfile.write(os.path.join(directory, "synthetic%d_%s.wav" % (i, k)), spec.FS, x)
    return find_triples(directory)


def table(rows, figures=FIGURES):
    """rows: dicts with snr_pos, snr_neg, lookahead and the means -> the printed table"""
    head = "%8s %8s %5s %6s" % ("snr_pos", "snr_neg", "L", "jobs") + "".join("%12s" % f for f in figures)
    lines = [head]
    for r in rows:
        lines.append("%8g %8g %5d %6d" % (r["snr_pos"], r["snr_neg"], r["lookahead"], r["jobs"]) + "".join("%12.4f" % r[f] for f in figures))
    return "\n".join(lines)


def summarise(results, lookahead, figures=FIGURES):
    """evaluate_corpus's records -> one row per SNR pair: the plain means of the improvements"""
    groups = {}
    for r in results:
        groups.setdefault((r["snr_pos"], r["snr_neg"]), []).append(r["improvement"])
    return [dict({"snr_pos": p, "snr_neg": n, "lookahead": lookahead, "jobs": len(g)},
                 **{f: float(np.mean([x[f] for x in g])) for f in figures}) for (p, n), g in sorted(groups.items())]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("directory", nargs="?")
    ap.add_argument("--snrs", default="-3,0,3,5,8", help="the grid: every (snr_pos, snr_neg) pair of these values")
    ap.add_argument("--lookaheads", default=str(spec.LOOKAHEAD))
    ap.add_argument("--weights", default="synthetic", choices=["synthetic", "checkpoint"])
    ap.add_argument("--json", default=None, help="also write the rows as JSON")
    ap.add_argument("--phase_iters", type=int, default=0, help="Griffin-Lim iterations on the denoised rows before their iSTFT (default 0)")
    ap.add_argument("--stoi", action="store_true", help="also the mean improvements of STOI and extended STOI: stoi_i, estoi_i")
    ap.add_argument("--bss", action="store_true", help="also the mean improvements of BSS Eval's SDR, SIR and SAR: sdr_i, sir_i, sar_i")
    ap.add_argument("--quality", action="store_true",
                    help="also the mean changes of LLR and cepstral distance (lower is better) and of fwSegSNR: llr_i, cd_i, fwsegsnr_i")
    a = ap.parse_args(argv)
    figures = FIGURES + (STOI_FIGURES if a.stoi else ()) + (BSS_FIGURES if a.bss else ()) + (QUALITY_FIGURES if a.quality else ())
    grid = [float(v) if "." in v else int(v) for v in a.snrs.split(",")]
    las = [int(v) for v in a.lookaheads.split(",")]
    for L in las:
        spec.check_lookahead(L)
    apply.FLAGS.weights = a.weights
    eng = engine.Engine(spec.DENOISER, apply._load_weights(spec.DENOISER) if a.weights == "checkpoint" else None, precision="f16x3")
    apply.set_engine(spec.DENOISER, eng)
    tmp = None
    try:
        if a.directory:
            triples = find_triples(a.directory)
        else:
            tmp = tempfile.TemporaryDirectory()
            triples = synthetic_triples(tmp.name)
        if not triples:
            raise SystemExit("no <name>_speech.wav in %s" % a.directory)
        pairs = [(p, n) for p in grid for n in grid]
        rows = []
        for L in las:
            rows += summarise(apply.evaluate_corpus(triples, snrs=pairs, lookahead=L, stoi=a.stoi, bss=a.bss, quality=a.quality, phase_iters=a.phase_iters), L, figures)
        print("%d triples x %d SNR pairs x %d look-aheads, weights: %s" % (len(triples), len(pairs), len(las), a.weights))
        print(table(rows, figures))
        if a.json:
            with open(a.json, "w") as f:
                json.dump({"triples": len(triples), "weights": a.weights, "rows": rows}, f, indent=1)
    finally:
        apply._engines.pop(spec.DENOISER, None)
        eng.close()
        if tmp is not None:
            tmp.cleanup()
    return 0


if __name__ == "__main__":
    sys.exit(main())
