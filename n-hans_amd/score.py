"""Scoring an output against a clean target: SI-SDR, SNR, segmental SNR of waveforms, the reference's training loss and
the log-spectral distance of log-magnitude rows (include/nhans_hip.h: nhans_score_*).

The device computes the figures (score.hip) -- Context.score / Engine.score_device / Engine.score_rows; this module
holds their names, the improvement of one record over another, and the float64 numpy DEFINITION the tests and the
documents measure the device against: `reference` and `reference_rows` form every sum with math.fsum, which is exact, so
the only roundings in them are the ones the definition names.  No torch here: the command line imports this."""
import math

import numpy as np

from . import spec

FIELDS = ("n", "See", "Stt", "Set", "Sdd", "alpha", "Srr", "snr_db", "si_sdr_db", "segsnr_db", "frames_counted",
          "frames_skipped")                                 # the first twelve of NHANS_SCORE_FIELDS doubles
ROW_FIELDS = ("frames", "loss", "lsd_db")                   # the first three of NHANS_SCORE_ROW_FIELDS doubles
FIGURES = ("si_sdr_db", "snr_db", "segsnr_db", "loss", "lsd_db")
SEG_LO, SEG_HI = -10.0, 35.0
LSD_SCALE = 20.0 / math.log(10.0)
IMP = np.linspace(2, 1, spec.BINS, dtype=np.float32)        # the reference's loss weights (SN/main.py:245-248)
_INTS = ("n", "frames", "frames_counted", "frames_skipped")


def record(values):
    """NHANS_SCORE_FIELDS doubles of one clip -> dict by name."""
    return {k: (int(values[i]) if k in _INTS else float(values[i])) for i, k in enumerate(FIELDS)}


def row_record(values):
    """NHANS_SCORE_ROW_FIELDS doubles of one clip -> dict by name."""
    return {k: (int(values[i]) if k in _INTS else float(values[i])) for i, k in enumerate(ROW_FIELDS)}


def improvement(before, after):
    """What `after` gains over `before`, both scored against the same target: the dB differences and the ratio of the
    losses (below one is better)."""
    out = {k[:-3] + "_i": after[k] - before[k] for k in ("si_sdr_db", "snr_db", "segsnr_db") if k in after and k in before}
    if "loss" in after and "loss" in before:
        with np.errstate(divide="ignore", invalid="ignore"):
            out["loss_ratio"] = float(np.float64(after["loss"]) / np.float64(before["loss"]))
    return out


def mean_of(records, keys=None):
    """The plain mean of every numeric figure over a list of records (directory mode's summary)."""
    keys = keys or [k for k in records[0] if isinstance(records[0][k], (int, float)) and k not in _INTS]
    return {k: float(np.mean([r[k] for r in records])) for k in keys}


# ---- the float64 definition -------------------------------------------------------------------------
def _db(q):
    """10 log10(q) by IEEE: 0 -> -inf, inf -> inf, negative or NaN -> NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(np.float64(q)))


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _fsum(x):
    """math.fsum, with IEEE's answer where it would raise (an infinity of each sign) or overflow."""
    try:
        return math.fsum(x)
    except (OverflowError, ValueError):
        with np.errstate(all="ignore"):
            return float(np.sum(np.asarray(x, dtype=np.float64)))


def _fma_neg(alpha, t, e):
    """fma(-alpha, t, e) for a double alpha and float32-valued t: alpha is split into two halves whose products with t
    are exact, and the three terms are added with error-free transformations (the last addition rounds once more, far
    below the rounding of the result itself)."""
    with np.errstate(all="ignore"):
        c = 134217729.0 * alpha
        hi = c - (c - alpha)
        if not math.isfinite(hi):
            return e - alpha * t
        lo = alpha - hi
        a, b = -hi * t, -lo * t

        def two_sum(x, y):
            s = x + y
            v = s - x
            return s, (x - (s - v)) + (y - v)

        s1, e1 = two_sum(e, a)
        s2, e2 = two_sum(s1, b)
        r = s2 + (e1 + e2)
        return np.where(np.isfinite(r), r, e - alpha * t)


def frame_snr(e, t, lo=SEG_LO, hi=SEG_HI):
    """Per frame of the network's framing (400 samples, hop 160): clamp(10 log10(Pt / Pd), lo, hi), 35 where Pd == 0, NaN
    where Pt == 0 -> (float64 [frames], bool [frames]: the frame was skipped)."""
    n = min(len(e), len(t))
    e, t = np.asarray(e[:n], dtype=np.float64), np.asarray(t[:n], dtype=np.float64)
    F = spec.frames_for_samples(n)[1]
    with np.errstate(all="ignore"):
        tt, dd = t * t, (e - t) * (e - t)
    out, skipped = np.empty(F, dtype=np.float64), np.zeros(F, dtype=bool)
    for f in range(F):
        pt = _fsum(tt[spec.HOP * f:spec.HOP * f + spec.WIN])
        pd = _fsum(dd[spec.HOP * f:spec.HOP * f + spec.WIN])
        if pt == 0.0:
            out[f], skipped[f] = np.nan, True
        elif pd == 0.0:
            out[f] = SEG_HI
        else:
            v = _db(_div(pt, pd))
            out[f] = lo if v < lo else (hi if v > hi else v)
    return out, skipped


def reference(e, t, frames=False):
    """The waveform figures of estimate e against target t (float32 values; scored over the common prefix), as the header
    defines them -> dict by FIELDS (frames=True: plus "frames", float64 [frames], NaN where the frame was skipped)."""
    n = min(len(e), len(t))
    e, t = np.asarray(e[:n], dtype=np.float32).astype(np.float64), np.asarray(t[:n], dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = e - t
        See, Stt, Set, Sdd = _fsum(e * e), _fsum(t * t), _fsum(e * t), _fsum(d * d)
        alpha = 0.0 if Stt == 0.0 else _div(Set, Stt)
        r = _fma_neg(alpha, t, e) if n else np.zeros(0)
        Srr = _fsum(r * r)
    seg, skipped = frame_snr(e, t)
    counted = seg[~skipped]
    out = {"n": n, "See": See, "Stt": Stt, "Set": Set, "Sdd": Sdd, "alpha": alpha, "Srr": Srr,
           "snr_db": float("nan") if Stt == 0.0 else _db(_div(Stt, Sdd)),
           "si_sdr_db": float("nan") if Stt == 0.0 else _db(_div(alpha * alpha * Stt, Srr)),
           "segsnr_db": _div(_fsum(counted), len(counted)) if len(counted) else float("nan"),
           "frames_counted": int(len(counted)), "frames_skipped": int(skipped.sum())}
    if frames:
        out["frames"] = seg
    return out


def reference_rows(E, T, frames=False, imp=IMP):
    """The row figures of two [frames, 201] float32 log-magnitude arrays -> dict by ROW_FIELDS (frames=True: plus
    "per_frame", float64 [frames, 2]: each frame's loss and lsd)."""
    E, T = np.asarray(E, dtype=np.float32).astype(np.float64), np.asarray(T, dtype=np.float32).astype(np.float64)
    F = E.shape[0]
    w = np.asarray(imp, dtype=np.float64)
    per = np.empty((F, 2), dtype=np.float64)
    with np.errstate(all="ignore"):
        d = E - T
        a, b = (d * d) * w[None, :], (LSD_SCALE * d) * (LSD_SCALE * d)
    for f in range(F):
        per[f, 0] = _fsum(a[f]) / spec.BINS
        per[f, 1] = math.sqrt(_fsum(b[f]) / spec.BINS) if np.isfinite(b[f]).all() else float(np.sqrt(np.sum(b[f]) / spec.BINS))
    out = {"frames": F, "loss": _fsum(per[:, 0]) / F if F else float("nan"), "lsd_db": _fsum(per[:, 1]) / F if F else float("nan")}
    if frames:
        out["per_frame"] = per
    return out


def features64(x):
    """The log-magnitude rows of a waveform in float64 numpy: 400-sample periodic Hann frames at hop 160, log(|rfft| +
    1e-5) -- what nhans_stft_features computes in float32.  (For the documents and the fixture; the device scores its
    own rows.)"""
    x = np.asarray(x, dtype=np.float64)
    F = spec.frames_for_samples(len(x))[1]
    idx = spec.HOP * np.arange(F)[:, None] + np.arange(spec.WIN)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(spec.WIN) / spec.WIN)
    return np.log(np.abs(np.fft.rfft(x[idx] * w[None, :], n=spec.WIN, axis=1)) + spec.LOG_EPS).reshape(F, spec.BINS)


def reference_all(e, t):
    """reference(e, t) plus the row figures of the two signals' float64 features (features64)."""
    n = min(len(e), len(t))
    out = reference(e, t)
    rows = reference_rows(features64(e[:n]).astype(np.float32), features64(t[:n]).astype(np.float32))
    out.update(loss=rows["loss"], lsd_db=rows["lsd_db"], frames=rows["frames"])
    return out
