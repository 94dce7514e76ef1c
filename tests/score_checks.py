"""What tests/test_score_host.py and tests/test_gpu_score.py share: the clips, the float64 bar and the planted faults.

The bar.  The reference (nhans_amd.score.reference / reference_rows) forms every sum with math.fsum, so it is exact up to
the roundings the definition itself names.  U = 2^-53.

  * A sum of n terms added in ANY fixed order is within n U sum|terms| of the exact sum.  A term carries at most four
    roundings on either side (the difference e - t, its square, a product with a constant or a weight, the reference's
    rounded term), so  |S - S_ref| <= (n + 4) U sum|terms|; for the sums of squares sum|terms| is S itself.
  * alpha = Set / Stt: relative error ea = rel(Set) + rel(Stt) + U (the division).
  * Srr = sum r^2, r = fma(-alpha, t, e): (n + 4) U Srr for the sum, and for the alpha it is formed with
    2 |alpha| ea |sum r t| + (alpha ea)^2 Stt  -- sum r t is zero but for rounding (r is orthogonal to t), and the helper
    takes it from the reference's own r, exactly.
  * A dB figure 10 log10(A / B): (10 / ln 10) (rel(A) + rel(B) + U) for its argument, plus 4 U |ref| for the logarithm
    and the product on both sides (one-ulp-class functions).  For SI-SDR, A = alpha^2 Stt: rel(A) = 2 ea + rel(Stt) + 2 U.
  * A frame's segmental value is a dB figure of two 400-term sums; the clamp is 1-Lipschitz and the decisions Pt == 0,
    Pd == 0 are exact on both sides (a sum of squares is zero only if every term is).  The mean over F counted frames adds
    (F + 1) U mean|v|.
  * A row's loss: 201 terms of (d d) imp, d = E - T exact in double for float32 rows of the network's domain: relative
    (201 + 4 + 1) U with the division.  Its lsd: half of that (the square root) plus U.  The clip's means add (F + 1) U.

C_BAR = 2 is the stated constant on all of it, for the second-order terms dropped above.  It is not tuned: the worst
measured ratio to the bar is in profiles/score/README.md, and a ratio above one half would be a defect to find.

Planted faults (test_score_host.py): each must leave the bar by orders of magnitude, so the bar is known to see them."""
import math

import numpy as np

from nhans_amd import hip, score, spec
from fbank_checks import HI, LO

U = 2.0 ** -53
C_BAR = 2.0
DB = 10.0 / math.log(10.0)
TILE = hip.SCORE_TILE                       # samples per workgroup of score.hip (kScoreTile)
LENGTHS = [1, 159, 160, 399, 400, 401, 559, 560, 561, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
ROW_COUNTS = [0, 1, 15, 16, 17]             # rows per clip around score.hip's 16-row tile (kScoreRowTile)
WAVE_FIGURES = ("See", "Stt", "Set", "Sdd", "alpha", "Srr", "snr_db", "si_sdr_db", "segsnr_db")
ROW_FIGURES = ("loss", "lsd_db")


# ---- clips ----------------------------------------------------------------------------------------
def clip(n, seed):
    """-> (estimate, target) float32 [n]: a target of speech-like level and an estimate 5 - 6 dB away from it."""
    rng = np.random.default_rng(1000 + seed)
    t = (0.3 * rng.standard_normal(n)).astype(np.float32)
    e = (0.9 * t + 0.15 * rng.standard_normal(n)).astype(np.float32)
    return e, t


def length_clips():
    return [clip(n, i) for i, n in enumerate(LENGTHS)]


def silent_frames_clip():
    """2,000 samples = 11 frames; the target is zero on [320, 1040): frames 2, 3 and 4 are silent (samples [320, 720),
    [480, 880) and [640, 1040)), their neighbours are not.  The estimate equals the target on [1280, 2000): frames 8 ... 10 have Pd == 0."""
    e, t = clip(2000, 77)
    t[320:1040] = 0.0
    e[1280:] = t[1280:]
    return e, t


def clamp_clip():
    """Three frames' worth: frame 0 far below -10 dB (estimate = 100 x target), frame 5 far above 35 dB."""
    e, t = clip(400 + 160 * 5, 78)
    e[:400] = 100.0 * t[:400]
    e[800:] = t[800:] * np.float32(1.0 + 2.0 ** -12)
    return e, t


def uniform_rows(n, seed):
    return np.random.default_rng(seed).uniform(LO, HI, size=(n, spec.BINS)).astype(np.float32)


def edge_rows(n):
    """all-LO against all-HI: the largest difference the domain holds, in every bin"""
    return np.full((n, spec.BINS), LO, np.float32), np.full((n, spec.BINS), HI, np.float32)


# ---- the bar --------------------------------------------------------------------------------------
def _rel_db(rel_arg, ref):
    return C_BAR * (DB * rel_arg + 4.0 * U * (abs(ref) if math.isfinite(ref) else 0.0))


def wave_bar(e, t):
    """-> (reference record with "frames", {figure: absolute bar}, per-frame bar [frames])"""
    ref = score.reference(e, t, frames=True)
    n = ref["n"]
    e64, t64 = np.asarray(e[:n], np.float64), np.asarray(t[:n], np.float64)
    k = (n + 4) * U
    abs_et = math.fsum(np.abs(e64 * t64))
    rel = {"See": k, "Stt": k, "Sdd": k}
    rel_set = k * abs_et / abs(ref["Set"]) if ref["Set"] != 0.0 else math.inf
    ea = rel_set + rel["Stt"] + U
    alpha = ref["alpha"]
    r = score._fma_neg(alpha, t64, e64) if n else np.zeros(0)
    srr_abs = k * ref["Srr"] + 2.0 * abs(alpha) * (ea if math.isfinite(ea) else 0.0) * abs(math.fsum(r * t64)) \
        + ((alpha * ea) ** 2 * ref["Stt"] if math.isfinite(ea) else 0.0)
    rel_srr = srr_abs / ref["Srr"] if ref["Srr"] > 0 else 0.0
    bar = {"See": C_BAR * k * ref["See"], "Stt": C_BAR * k * ref["Stt"], "Sdd": C_BAR * k * ref["Sdd"],
           "Set": C_BAR * k * abs_et, "alpha": C_BAR * (abs(alpha) * ea if math.isfinite(ea) else k * abs_et / max(ref["Stt"], 1e-300)),
           "Srr": C_BAR * srr_abs,
           "snr_db": _rel_db(rel["Stt"] + rel["Sdd"] + U, ref["snr_db"]),
           "si_sdr_db": _rel_db((2.0 * ea if math.isfinite(ea) else 0.0) + rel["Stt"] + 2.0 * U + rel_srr + U, ref["si_sdr_db"])}
    fr = ref["frames"]
    per = np.array([_rel_db(2.0 * (spec.WIN + 4) * U + U, v) if math.isfinite(v) else 0.0 for v in fr])
    cnt = ref["frames_counted"]
    if cnt:
        v = fr[np.isfinite(fr)]
        bar["segsnr_db"] = float(per[np.isfinite(fr)].mean()) + C_BAR * (cnt + 1) * U * float(np.abs(v).mean())
    else:
        bar["segsnr_db"] = 0.0
    return ref, bar, per


def rows_bar(E, T):
    """-> (reference record with "per_frame", {figure: absolute bar}, per-frame bars [frames, 2])"""
    ref = score.reference_rows(E, T, frames=True)
    F = ref["frames"]
    k_loss, k_lsd = (spec.BINS + 5) * U, (0.5 * (spec.BINS + 6) + 1.0) * U
    per = C_BAR * ref["per_frame"] * np.array([k_loss, k_lsd])[None, :]
    bar = {"loss": C_BAR * (k_loss + (F + 1) * U) * ref["loss"] if F else 0.0,
           "lsd_db": C_BAR * (k_lsd + (F + 1) * U) * ref["lsd_db"] if F else 0.0}
    return ref, bar, per


def ratio(got, ref, bar):
    """|got - ref| / bar; values that are not finite must be THE SAME non-finite value (ratio 0), else inf."""
    got, ref = float(got), float(ref)
    if not (math.isfinite(got) and math.isfinite(ref)):
        same = (math.isnan(got) and math.isnan(ref)) or got == ref
        return 0.0 if same else math.inf
    if got == ref:
        return 0.0
    return abs(got - ref) / bar if bar > 0 else math.inf


def wave_ratios(got, e, t):
    """got: dict by score.FIELDS (+ optional "frames") -> {figure: ratio to the bar}; the counts must be equal."""
    ref, bar, per = wave_bar(e, t)
    for k in ("n", "frames_counted", "frames_skipped"):
        assert int(got[k]) == ref[k], (k, got[k], ref[k])
    out = {k: ratio(got[k], ref[k], bar[k]) for k in WAVE_FIGURES}
    if "frames" in got:
        out["frames"] = max([ratio(g, r, b) for g, r, b in zip(got["frames"], ref["frames"], per)], default=0.0)
    return out


def rows_ratios(got, E, T):
    ref, bar, per = rows_bar(E, T)
    assert int(got["frames"]) == ref["frames"]
    out = {k: ratio(got[k], ref[k], bar[k]) for k in ROW_FIGURES}
    if "per_frame" in got:
        out["per_frame"] = max([ratio(g, r, b) for g, r, b in zip(np.ravel(got["per_frame"]), np.ravel(ref["per_frame"]),
                                                                 np.ravel(per))], default=0.0)
    return out


# ---- planted faults -------------------------------------------------------------------------------
def fault_dropped_last_sample(e, t):
    return score.reference(e[:-1], t[:-1])


def fault_frame_count_off_by_one(e, t):
    """the segmental mean over one frame too few"""
    out = score.reference(e, t)
    seg, skipped = score.frame_snr(e, t)
    v = seg[:-1][~skipped[:-1]]
    out["segsnr_db"] = math.fsum(v) / len(v)
    return out


def fault_clamp_after_mean(e, t):
    out = score.reference(e, t)
    seg, skipped = score.frame_snr(e, t, lo=-math.inf, hi=math.inf)
    m = math.fsum(seg[~skipped]) / int((~skipped).sum())
    out["segsnr_db"] = min(max(m, score.SEG_LO), score.SEG_HI)
    return out


def fault_imp_reversed(E, T):
    return score.reference_rows(E, T, imp=score.IMP[::-1])
