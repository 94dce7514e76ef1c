"""Scoring an output against a clean target: SI-SDR, SNR, segmental SNR of waveforms, the reference's training loss and
the log-spectral distance of log-magnitude rows (include/nhans_hip.h: nhans_score_*).

The device computes the figures (score.hip) -- Context.score / Engine.score_device / Engine.score_rows; this module
holds their names, the improvement of one record over another, and the float64 numpy DEFINITION the tests and the
documents measure the device against: `reference` and `reference_rows` form every sum with math.fsum, which is exact, so
the only roundings in them are the ones the definition names.  STOI and extended STOI (stoi.hip: Context.stoi /
Engine.stoi_device) have theirs in `stoi_reference`, built from the steps below it, and BSS
Eval's SDR, SIR and SAR (bsseval.hip: Context.bss_eval / Engine.bss_eval_device) in
`bss_reference`.  Delay estimation for signals that are not aligned (align.hip: Context.align, Context.score(align=...);
DESIGN.md section 1.13) has its definition in `align_reference`.  LLR, cepstral distance and frequency-weighted
segmental SNR (quality.hip: Context.quality / Engine.quality_device) have theirs in
`quality_reference`.  Drift-aware alignment for signals recorded on two clocks (drift.hip: Context.align_drift,
Context.score(align=..., drift=True)) has its definition in `drift_reference`, `drift_fit` and
`drift_warp_reference`.  No torch here: the command line imports this."""
import functools
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
STOI_FIELDS = ("n", "frames", "frames_kept", "segments", "stoi", "estoi")     # the first six of NHANS_STOI_FIELDS doubles
# third-octave bands from 150 Hz as bins [lo, hi) of the 512-point transform at 10 kHz (stoi_band_table re-derives them)
STOI_BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
              (87, 109), (109, 138), (138, 174), (174, 219))
STOI_RATE, STOI_FRAME, STOI_HOP, STOI_FFT, STOI_SEGMENT = 10000, 256, 128, 512, 30
STOI_EPS = 2.0 ** -52
STOI_CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
STOI_RANGE = 1e-4                                           # 40 dB
BSS_FIELDS = ("n", "J", "L", "E_e", "E_tgt", "E_int", "E_art", "E_dist", "E_ti", "sdr_db", "sir_db", "sar_db",
              "singular")                                   # the first thirteen of NHANS_BSS_FIELDS doubles
BSS_ENERGIES, BSS_FIGURES = BSS_FIELDS[3:9], BSS_FIELDS[9:12]
BSS_MAX_FILTER = 512
ALIGN_FIELDS = ("ne", "nt", "D", "delay", "c_peak", "rho", "n_common")        # the first seven of NHANS_ALIGN_FIELDS doubles
ALIGN_MAX_LAG = 16000
QUALITY_FIELDS = ("n", "frames", "frames_lpc", "frames_fw", "llr", "llr_95", "cd_db", "cd_95_db",
                  "fwsegsnr_db")                            # the first nine of NHANS_QUALITY_FIELDS doubles
QUALITY_FIGURES = QUALITY_FIELDS[4:]
QUALITY_FRAME, QUALITY_HOP, QUALITY_ORDER, QUALITY_FFT, QUALITY_BINS = 480, 120, 16, 512, 257
QUALITY_BANDS, QUALITY_MAX_BANDS = 25, 32
QUALITY_LLR_MAX, QUALITY_CD_MAX, QUALITY_CD_SCALE = 2.0, 10.0, 4.342944819032518      # 10 / ln 10
QUALITY_SNR_MIN, QUALITY_SNR_MAX, QUALITY_GAMMA = -10.0, 35.0, 0.2
_INTS = ("n", "frames", "frames_counted", "frames_skipped", "frames_kept", "segments", "stoi_n", "stoi_frames", "J", "L", "singular",
         "bss_n", "ne", "nt", "D", "delay", "n_common", "frames_lpc", "frames_fw", "quality_n", "quality_frames")


def record(values, fields=FIELDS):
    """The doubles of one clip's record (NHANS_SCORE_FIELDS of them; NHANS_<FAMILY>_FIELDS with that family's names as
    `fields`) -> dict by name."""
    return {k: (int(values[i]) if k in _INTS else float(values[i])) for i, k in enumerate(fields)}


row_record = functools.partial(record, fields=ROW_FIELDS)
stoi_record = functools.partial(record, fields=STOI_FIELDS)
bss_record = functools.partial(record, fields=BSS_FIELDS)
align_record = functools.partial(record, fields=ALIGN_FIELDS)
quality_record = functools.partial(record, fields=QUALITY_FIELDS)


def merge(rec, other, prefix):
    """A score record with another family's figures of the same pair merged in; a name the record already has (n, frames:
    there the 16 kHz samples and the STFT rows) takes the prefix: stoi_n, stoi_frames, bss_n, quality_n, quality_frames."""
    return dict(rec, **{(prefix + k if k in rec else k): v for k, v in other.items()})


merge_stoi = functools.partial(merge, prefix="stoi_")
merge_bss = functools.partial(merge, prefix="bss_")
merge_quality = functools.partial(merge, prefix="quality_")


def improvement(before, after):
    """What `after` gains over `before`, both scored against the same target: the dB differences and the ratio of the
    losses (below one is better); where both carry STOI figures, their differences stoi_i and estoi_i too; where both
    carry BSS Eval figures, sdr_i, sir_i and sar_i; where both carry the quality figures, the plain differences llr_i,
    llr_95_i, cd_i, cd_95_i (LOWER is better for these four: an improvement is negative) and fwsegsnr_i."""
    out = {k[:-3] + "_i": after[k] - before[k] for k in ("si_sdr_db", "snr_db", "segsnr_db") if k in after and k in before}
    if "stoi" in after and "stoi" in before:
        out.update(stoi_i=after["stoi"] - before["stoi"], estoi_i=after["estoi"] - before["estoi"])
    if all(k in after and k in before for k in BSS_FIGURES):
        with np.errstate(invalid="ignore"):
            out.update({k[:-3] + "_i": float(np.float64(after[k]) - np.float64(before[k])) for k in BSS_FIGURES})
    if all(k in after and k in before for k in QUALITY_FIGURES):
        with np.errstate(invalid="ignore"):
            out.update({(k[:-3] if k.endswith("_db") else k) + "_i": float(np.float64(after[k]) - np.float64(before[k]))
                        for k in QUALITY_FIGURES})
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


# ---- STOI and extended STOI: the float64 definition (include/nhans_hip.h) ----------------------------
def stoi_out_count(n16):
    """samples at 10 kHz of n16 samples at 16 kHz: ceil(5 n / 8) (nhans_stoi_out_count)"""
    return -((-5 * int(n16)) // 8)


def stoi_band_table(rate=STOI_RATE, nfft=STOI_FFT, nbands=len(STOI_BANDS), first=150.0):
    """The bands from their formula: the bins of linspace(0, rate, nfft + 1) nearest to first * 2^(j/3) * 2^(-+1/6)."""
    f = np.linspace(0, rate, nfft + 1)[:nfft // 2 + 1]
    cf = first * 2.0 ** (np.arange(nbands) / 3.0)
    lo, hi = cf * 2.0 ** (-1.0 / 6.0), cf * 2.0 ** (1.0 / 6.0)
    return tuple((int(np.argmin(np.square(f - a))), int(np.argmin(np.square(f - b)))) for a, b in zip(lo, hi))


def stoi_window():
    """hanning(256): the 256 inner points of a 258-point symmetric Hann window"""
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(STOI_FRAME) + 1.0) / (STOI_FRAME + 1.0)))


def stoi_num_frames(n):
    return -((STOI_FRAME - int(n)) // STOI_HOP) if n > STOI_FRAME else 0


def stoi_frames(x, w):
    """-> float64 [M0, 256]: the frames of x at hop 128, each times w (a final frame that would end at len(x) is not taken)"""
    x = np.asarray(x, dtype=np.float64)
    M = stoi_num_frames(len(x))
    idx = STOI_HOP * np.arange(M)[:, None] + np.arange(STOI_FRAME)[None, :]
    return x[idx] * w[None, :] if M else np.zeros((0, STOI_FRAME))


def stoi_keep(frames):
    """windowed frames -> (bool [M0]: P_m > P_max * 1e-4, the powers P_m)"""
    p = np.array([_fsum(f * f) for f in frames], dtype=np.float64)
    return (p > p.max() * STOI_RANGE if len(p) else np.zeros(0, bool)), p


def stoi_rejoin(frames):
    """kept windowed frames [Mk, 256] -> their overlap-add at hop 128, 128 (Mk - 1) + 256 samples (none for Mk == 0)"""
    out = np.zeros(STOI_HOP * (len(frames) - 1) + STOI_FRAME if len(frames) else 0)
    for k, f in enumerate(frames):
        out[STOI_HOP * k:STOI_HOP * k + STOI_FRAME] += f
    return out


def stoi_bands_of(frames, bands=STOI_BANDS):
    """windowed analysis frames [Mf, 256] -> float64 [Mf, 15]: sqrt of each band's summed |rfft(frame, 512)|^2"""
    X = np.fft.rfft(frames, n=STOI_FFT, axis=1) if len(frames) else np.zeros((0, STOI_FFT // 2 + 1), complex)
    p = X.real * X.real + X.imag * X.imag
    return np.array([[math.sqrt(_fsum(row[lo:hi])) for lo, hi in bands] for row in p], dtype=np.float64).reshape(len(frames), len(bands))


def _unit(v):
    """v (1-D) made zero-mean and divided by its norm + eps"""
    c = v - _fsum(v) / len(v)
    return c / (math.sqrt(_fsum(c * c)) + STOI_EPS)


def stoi_segment(X, Y, clip=STOI_CLIP):
    """[30, 15] band values of the target and of the estimate -> d_s"""
    terms = []
    for j in range(X.shape[1]):
        x, y = X[:, j], Y[:, j]
        a = math.sqrt(_fsum(x * x)) / (math.sqrt(_fsum(y * y)) + STOI_EPS)
        terms.append(_unit(x) * _unit(np.minimum(a * y, clip * x)))
    return _fsum(np.concatenate(terms)) / X.shape[1]


def estoi_segment(X, Y):
    """[30, 15] band values of the target and of the estimate -> e_s: rows (bands) normalised, then columns"""
    def both(A):
        R = np.stack([_unit(A[:, j]) for j in range(A.shape[1])], axis=1)
        return np.stack([_unit(R[q]) for q in range(A.shape[0])], axis=0)
    return _fsum((both(X) * both(Y)).ravel()) / X.shape[0]


def stoi_reference(e10, t10, per_segment=False):
    """STOI and extended STOI of estimate e10 against target t10 (float32 values at 10 kHz; scored over the common prefix)
    as the header defines them -> dict by STOI_FIELDS (per_segment=True: plus "per_segment", float64 [segments, 2] = d_s,
    e_s)."""
    n = min(len(e10), len(t10))
    e, t = np.asarray(e10[:n], dtype=np.float32).astype(np.float64), np.asarray(t10[:n], dtype=np.float32).astype(np.float64)
    w = stoi_window()
    ft, fe = stoi_frames(t, w), stoi_frames(e, w)
    keep, _ = stoi_keep(ft)
    X = stoi_bands_of(stoi_frames(stoi_rejoin(ft[keep]), w))
    Y = stoi_bands_of(stoi_frames(stoi_rejoin(fe[keep]), w))
    S = max(len(X) - STOI_SEGMENT + 1, 0)
    per = np.array([[stoi_segment(X[s:s + STOI_SEGMENT], Y[s:s + STOI_SEGMENT]),
                     estoi_segment(X[s:s + STOI_SEGMENT], Y[s:s + STOI_SEGMENT])] for s in range(S)], dtype=np.float64).reshape(S, 2)
    out = {"n": n, "frames": len(ft), "frames_kept": int(keep.sum()), "segments": S,
           "stoi": _fsum(per[:, 0]) / S if S else float("nan"), "estoi": _fsum(per[:, 1]) / S if S else float("nan")}
    if per_segment:
        out["per_segment"] = per
    return out


# ---- BSS Eval: the float64 definition (include/nhans_hip.h: nhans_bss_eval) --------------------------
def _lag_sum(a, b, d):
    """sum_t a[t] b[t + d], exactly rounded (the products of float32 values are exact in double)"""
    n = len(a)
    if d >= 0:
        return _fsum((a[:n - d] * b[d:]).tolist()) if d < n else 0.0
    return _fsum((a[-d:] * b[:n + d]).tolist()) if -d < n else 0.0


def bss_correlations(e, sources, L):
    """float64 arrays of float32 values, all n long -> (r, q): r[j][k] = float64 [2 L - 1], r_jk[d] at index d + L - 1;
    q[k] = float64 [L]"""
    J = len(sources)
    r = [[None] * J for _ in range(J)]
    for j in range(J):
        pos = np.array([_lag_sum(sources[j], sources[j], d) for d in range(L)])
        r[j][j] = np.concatenate([pos[:0:-1], pos])
        for k in range(j + 1, J):
            r[j][k] = np.array([_lag_sum(sources[j], sources[k], d) for d in range(-(L - 1), L)])
            r[k][j] = r[j][k][::-1].copy()
    q = [np.array([_lag_sum(s, e, b) for b in range(L)]) for s in sources]
    return r, q


def bss_gram(r, q, L):
    """-> (G [J L, J L], D [J L]): G[(j,a),(k,b)] = r_jk[a - b], D[(k,b)] = q_k[b]"""
    J = len(q)
    idx = np.arange(L)[:, None] - np.arange(L)[None, :] + (L - 1)
    G = np.block([[r[j][k][idx] for k in range(J)] for j in range(J)])
    return G, np.concatenate(q)


def bss_pivot_margin(G, R):
    """The least ratio of a pivot R_kk^2 of the lower factor R to the singular threshold J L 2^-52 G_kk (0 where a pivot is
    not finite or G_kk is 0)."""
    with np.errstate(all="ignore"):
        piv, thr = np.diag(R) ** 2, len(G) * 2.0 ** -52 * np.diag(G)
        m = np.where(np.isfinite(piv) & (thr > 0), piv / thr, 0.0)
    return float(m.min()) if len(m) else 0.0


def bss_solve(G, D, L):
    """-> (C, C0, pivot margin), or None where the clip is singular by the header's pivot rule"""
    from scipy.linalg import cho_factor, cho_solve
    try:
        with np.errstate(all="ignore"):
            R = np.tril(cho_factor(G, lower=True, check_finite=False)[0])
    except (np.linalg.LinAlgError, ValueError):
        return None
    margin = bss_pivot_margin(G, R)
    if not margin > 1.0:
        return None
    return cho_solve((R, True), D, check_finite=False), cho_solve((R[:L, :L], True), D[:L], check_finite=False), margin


def bss_project(C, C0, sources, L):
    """-> (P, s_target), float64 [n + L - 1]"""
    P = np.zeros(len(sources[0]) + L - 1)
    for k, s in enumerate(sources):
        P = P + np.convolve(C[k * L:(k + 1) * L], s)
    return P, np.convolve(C0, sources[0])


def bss_figures(e, P, st, L):
    """the energies and figures of the record from the projections"""
    ep = np.concatenate([e, np.zeros(L - 1)])
    ei, ea = P - st, ep - P
    sq = lambda v: _fsum((v * v).tolist())
    out = {"E_e": sq(ep), "E_tgt": sq(st), "E_int": sq(ei), "E_art": sq(ea), "E_dist": sq(ep - st), "E_ti": sq(st + ei)}
    out.update(sdr_db=_db(_div(out["E_tgt"], out["E_dist"])), sir_db=_db(_div(out["E_tgt"], out["E_int"])),
               sar_db=_db(_div(out["E_ti"], out["E_art"])))
    return out


def bss_reference(e, sources, filt_len=BSS_MAX_FILTER, filters=False):
    """SDR, SIR and SAR of estimate e against sources = [target] or [target, interferer] (float32 values; every signal cut
    to the common length) with filters of filt_len taps, as the header defines them -> dict by BSS_FIELDS (filters=True:
    plus "C", float64 [J, L], "C0", float64 [L], "G", "D" and "pivot_margin": the least ratio of a pivot to the singular
    threshold).  The correlations are exactly rounded (math.fsum), the solve is scipy's Cholesky, the projections
    np.convolve.  A singular clip (a clip of no samples is one): NaN for every energy and figure, singular = 1."""
    L, J = int(filt_len), len(sources)
    if J not in (1, 2) or not 1 <= L <= BSS_MAX_FILTER:
        raise ValueError("bss_reference: one or two sources and a filter of 1 ... %d taps" % BSS_MAX_FILTER)
    n = min([len(e)] + [len(s) for s in sources])
    e = np.asarray(e[:n], dtype=np.float32).astype(np.float64)
    src = [np.asarray(s[:n], dtype=np.float32).astype(np.float64) for s in sources]
    out = dict({"n": n, "J": J, "L": L}, **{k: float("nan") for k in BSS_ENERGIES + BSS_FIGURES})
    out["singular"] = 1
    G, D = bss_gram(*bss_correlations(e, src, L), L)
    sol = bss_solve(G, D, L) if n else None
    if sol is not None:
        C, C0, margin = sol
        P, st = bss_project(C, C0, src, L)
        out.update(bss_figures(e, P, st, L), singular=0)
    if filters:
        out.update(G=G, D=D, C=C.reshape(J, L) if sol else None, C0=C0 if sol else None, pivot_margin=margin if sol else 0.0)
    return out


# ---- delay estimation: the float64 definition (include/nhans_hip.h: nhans_align) -----------------------
def align_common(ne, nt, delay):
    """The samples a pair of ne and nt samples has in common once the estimate is taken to be `delay` samples late."""
    return max(0, min(ne - max(delay, 0), nt - max(-delay, 0)))


def align_lag_sum(e, t, d):
    """c[d] = sum_u e[u + d] t[u] over u in [max(0, -d), min(nt, ne - d)), exactly rounded (float64 arrays of float32
    values: the products are exact); an empty range gives +0.0"""
    lo, hi = max(0, -d), min(len(t), len(e) - d)
    return _fsum((e[lo + d:hi + d] * t[lo:hi]).tolist()) if hi > lo else 0.0


def align_pick(c, max_lag):
    """The lag of the largest of c[-D] ... c[D] (lag -D first): of equal values the smaller |d|, of -d and +d the
    non-negative one."""
    D = int(max_lag)
    best = 0
    for d in sorted(range(-D, D + 1), key=lambda d: (abs(d), -d)):      # 0, +1, -1, +2, -2, ...: the first of equals stays
        if c[d + D] > c[best + D]:
            best = d
    return best


def align_reference(e, t, max_lag, corr=False):
    """The delay of estimate e against target t (float32 values) within max_lag samples either way, as the header defines
    it -> dict by ALIGN_FIELDS: delay > 0 means the estimate is late, e[u + delay] lines up with t[u].  Every sum is exactly
    rounded (math.fsum of the exact products).  corr=True: plus "corr", float64 [2 max_lag + 1], lag -max_lag first."""
    D = int(max_lag)
    if not 0 <= D <= ALIGN_MAX_LAG:
        raise ValueError("align_reference: max_lag 0 ... %d" % ALIGN_MAX_LAG)
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    t = np.asarray(t, dtype=np.float32).astype(np.float64)
    c = np.array([align_lag_sum(e, t, d) for d in range(-D, D + 1)])
    delay = align_pick(c, D)
    See, Stt = _fsum((e * e).tolist()), _fsum((t * t).tolist())
    with np.errstate(all="ignore"):
        rho = float(np.float64(c[delay + D]) / np.sqrt(np.float64(See) * np.float64(Stt)))
    out = {"ne": len(e), "nt": len(t), "D": D, "delay": delay, "c_peak": float(c[delay + D]), "rho": rho,
           "n_common": align_common(len(e), len(t), delay)}
    if corr:
        out["corr"] = c
    return out


def align_cut(e, t, delay):
    """-> (e[max(delay, 0):][:n], t[max(-delay, 0):][:n]), n the common count: the pair with the estimate's delay taken out.
    A delay of more than the clip it shortens is an error, as the library has it."""
    d = int(delay)
    if d > len(e) or -d > len(t):
        raise ValueError("align_cut: delay %d is more than the %d samples of the %s it shortens"
                         % (d, len(e) if d > 0 else len(t), "estimate" if d > 0 else "target"))
    n = align_common(len(e), len(t), d)
    return e[max(d, 0):max(d, 0) + n], t[max(-d, 0):max(-d, 0) + n]


# ---- drift-aware alignment: the float64 definition (include/nhans_hip.h: nhans_drift_*) -----------------
# Target sample u lines up with position p(u) = a + u + b u of the estimate (a > 0: the estimate is late; b > 0: its clock
# runs fast).  Every operation is one IEEE double operation rounded to nearest; `_fma` is the fused multiply-add.
#   table      T = 16, Q = 512: G[q][k] = sinc(x) kaiser(x / T; beta = 10), x = k - q / Q, q = 0 ... Q, k = -T + 1 ... T (column
#              k + T - 1); row 0 the exact unit impulse; D[q] = G[q + 1] - G[q]  (drift_table; drift_library_table: the library's)
#   segments   blocks of B = 4096 target samples at hop H = 2048, J = (nt - B) // H + 1 of them (0 for nt < B); segment j's
#              centre lag z_j = floor(fma(cb, j H + (B - 1) / 2, ca) + 0.5)  (drift_centres)
#   lag vector c_j[d] = sum_i e[j H + i + d] t[j H + i], d in [z_j - R - T, z_j + R + T]; exactly rounded here (math.fsum of the exact
#              products), a fixed order of its own on the device
#   integer    d* in [z_j - R, z_j + R]: the largest c_j[d], then the smaller |d - z_j|, then the larger d
#   fine peak  v_k at d* + k / 32, k = -32 ... 32: w = floor(k / 32), r = k - 32 w, the chain acc = fma(c_j[d* + w + i], G[16 r][i], acc)
#              over i = -T + 1 ... T from +0.0 (a lag outside the vector is passed over); the best k: larger value, smaller |k|,
#              larger k; for |k| < 32: den = (v_{k-1} - 2 v_k) + v_{k+1}, delta = ((v_{k-1} - v_{k+1}) / (2 den)) / 32 clamped to
#              +-1/64 where den < 0, else 0; tau_j = (d* + k / 32) + delta
#   abscissa   u_j = j H + (sum_i i t_i^2) / E_t, E_t = sum_i t_i^2 over the block (exactly rounded sums here)
#   confidence rho_j = v_k / sqrt(E_e E_t), E_e = sum_i e[j H + i + d*]^2
#   flags      1: d* = z_j -+ R or k = -+32;  2: E_t == 0 or E_e == 0
#   fit        drift_fit: weighted least squares of tau on u, weights E_t, over the segments with flags == 0 and rho >= rho_min;
#              one trimming pass at `trim` samples; every sum ascending, every product rounded by itself -- nhans_drift_fit
#              restated operation by operation
#   warp       drift_warp_reference: y[u] = float32(chain over k of fma(e[m + k], g_k, acc)), p = fma(b, u, a) + u, m = floor(p),
#              f = (p - m) Q, q = min(floor(f), Q - 1), g_k = fma(f - q, D[q][k], G[q][k]), over [u_lo, u_hi) = drift_range
DRIFT_FIELDS = ("u", "tau", "rho", "E_t", "v_peak", "d_int", "flags", "z")     # the NHANS_DRIFT_FIELDS doubles of a segment
DRIFT_FIT_FIELDS = ("a", "b", "n_valid", "n_used", "rms_residual", "fit_ok")   # the NHANS_DRIFT_FIT_FIELDS doubles of a fit
DRIFT_T, DRIFT_Q, DRIFT_BLOCK, DRIFT_HOP, DRIFT_MAX_RADIUS, DRIFT_FINE = 16, 512, 4096, 2048, 1024, 32
DRIFT_MAX_SLOPE, DRIFT_MAX_DELAY = 2.0 ** -10, 2.0 ** 31
DRIFT_RHO_MIN, DRIFT_TRIM = 0.3, 1.0
DRIFT_EDGE, DRIFT_SILENT = 1, 2


def _two_sum(x, y):
    s = x + y
    v = s - x
    return s, (x - (s - v)) + (y - v)


def _fma(a, b, c):
    """fma(a, b, c) = a b + c rounded once, elementwise on float64 arrays (Boldo & Melquiond 2008: the product split exactly
    by Dekker, two error-free sums, the two errors added with rounding to odd, one last rounded sum).  Exact while nothing
    overflows or falls below 2^-969; a lane that is not finite gets a b + c."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        uh = a * b
        sa, sb = 134217729.0 * a, 134217729.0 * b
        ah, bh = sa - (sa - a), sb - (sb - b)
        al, bl = a - ah, b - bh
        ul = al * bl - (((uh - ah * bh) - al * bh) - ah * bl)
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        s, err = _two_sum(tl, vl)
        even = (s.view(np.int64) & 1) == 0
        up = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        z = np.where((err != 0) & even, up, s)
        r = vh + z
        return np.where(np.isfinite(r) & np.isfinite(uh), r, a * b + c)


def _bessel_i0(x):
    """the power series sum_k ((x / 2)^k / k!)^2 of the library's design, elementwise"""
    q = 0.25 * np.asarray(x, np.float64) ** 2
    term, total = np.ones_like(q), np.ones_like(q)
    for k in range(1, 200):
        term = term * (q / (float(k) * float(k)))
        total = total + term
        if np.all(term < total * 1e-18):
            break
    return total


@functools.lru_cache(maxsize=None)
def drift_table():
    """-> (G float64 [Q + 1, 2 T], D float64 [Q, 2 T]): the numpy design of the interpolation table"""
    T, Q = DRIFT_T, DRIFT_Q
    k = np.arange(-T + 1, T + 1, dtype=np.float64)[None, :]
    x = k - np.arange(Q + 1, dtype=np.float64)[:, None] / Q
    G = np.sinc(x) * (_bessel_i0(10.0 * np.sqrt(np.maximum(0.0, 1.0 - (x / T) ** 2))) / _bessel_i0(10.0))
    G[0] = 0.0
    G[0, T - 1] = 1.0
    G.setflags(write=False)
    D = G[1:] - G[:-1]
    D.setflags(write=False)
    return G, D


_drift_library_table = None


def drift_library_table():
    """-> (G, D): the very table the library uploads (nhans_drift_table, host only)"""
    global _drift_library_table
    if _drift_library_table is None:
        import ctypes
        from . import hip
        T2, Q = 2 * DRIFT_T, DRIFT_Q
        G, D = np.zeros((Q + 1, T2)), np.zeros((Q, T2))
        dp = ctypes.POINTER(ctypes.c_double)
        hip.check(hip.load().nhans_drift_table(G.ctypes.data_as(dp), D.ctypes.data_as(dp)))
        _drift_library_table = (G, D)
    return _drift_library_table


def drift_segments(nt):
    return (int(nt) - DRIFT_BLOCK) // DRIFT_HOP + 1 if nt >= DRIFT_BLOCK else 0


def drift_centres(ca, cb, J):
    """-> the J centre lags z_j of the line (ca, cb), Python ints"""
    x = np.arange(J, dtype=np.float64) * DRIFT_HOP + 0.5 * (DRIFT_BLOCK - 1)
    return [int(v) for v in np.floor(_fma(float(cb), x, float(ca)) + 0.5)]


def drift_pos(a, b, u):
    """p(u) = fma(b, u, a) + u, elementwise"""
    u = np.asarray(u, np.float64)
    return _fma(float(b), u, float(a)) + u


def _drift_line_check(who, a, b):
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError("%s: the line (%r, %r) is not finite" % (who, a, b))
    if abs(b) > DRIFT_MAX_SLOPE:
        raise ValueError("%s: drift %r is outside -2^-10 ... 2^-10" % (who, b))
    if abs(a) > DRIFT_MAX_DELAY:
        raise ValueError("%s: delay %r leaves the int32 range" % (who, a))


def drift_range(ne, nt, a, b):
    """-> (u_lo, u_hi): the maximal range of [0, nt) with 0 <= p(u) <= ne - 1, by bisection (p is strictly increasing);
    (0, 0) where it is empty"""
    _drift_line_check("drift_range", a, b)
    if ne <= 0 or nt <= 0:
        return 0, 0

    def first(pred):
        lo, hi = 0, int(nt)
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(float(drift_pos(a, b, float(mid)))):
                hi = mid
            else:
                lo = mid + 1
        return lo

    u_lo, u_hi = first(lambda p: p >= 0.0), first(lambda p: p > float(ne - 1))
    return (u_lo, u_hi) if u_hi > u_lo else (0, 0)


def drift_before(v, d, bv, bd):
    """(v, d) before (bv, bd): the larger value, then the smaller |d|, then the larger d"""
    if v != bv:
        return v > bv
    return abs(d) < abs(bd) if abs(d) != abs(bd) else d > bd


def drift_fine(c, lm, G):
    """The 65 fine values around the lag at index lm of the lag vector c (float64), each one fma chain over the taps ->
    float64 [65]"""
    T, F = DRIFT_T, DRIFT_FINE
    k = np.arange(-F, F + 1)
    w = k // F
    rows = G[(DRIFT_Q // F) * (k - F * w)]                   # [65, 2 T]
    acc = np.zeros(len(k))
    for j in range(2 * T):
        l = lm + w + j - (T - 1)
        ok = (l >= 0) & (l < len(c))
        acc = np.where(ok, _fma(c[np.clip(l, 0, len(c) - 1)], rows[:, j], acc), acc)
    return acc


def drift_peak(c, R, z, Et, Ee_of, u0, N, G):
    """What a segment's record is made of, from its lag vector c (lag z - R - T first), its energy Et and first moment N, and
    Ee_of(d*) -> the estimate's energy paired at d*: the record as the device forms it, operation by operation."""
    T, F = DRIFT_T, DRIFT_FINE
    best, bv = None, None
    for r in range(-R, R + 1):
        v = float(c[r + R + T])
        if best is None or drift_before(v, r, bv, best):
            best, bv = r, v
    fine = drift_fine(np.asarray(c, np.float64), best + R + T, G)
    fk, fv = None, None
    for i in range(2 * F + 1):
        if fk is None or drift_before(float(fine[i]), i - F, fv, fk):
            fk, fv = i - F, float(fine[i])
    delta = 0.0
    if -F < fk < F:
        vm, vp = float(fine[fk + F - 1]), float(fine[fk + F + 1])
        den = (vm - 2.0 * fv) + vp
        if den < 0.0:
            delta = min(max(((vm - vp) / (2.0 * den)) / F, -0.5 / F), 0.5 / F)
    dstar = z + best
    Ee = Ee_of(dstar)
    flags = (DRIFT_EDGE if abs(best) == R or abs(fk) == F else 0) | (DRIFT_SILENT if Et == 0.0 or Ee == 0.0 else 0)
    with np.errstate(all="ignore"):
        u = float(np.float64(u0) + np.float64(N) / np.float64(Et))
        rho = float(np.float64(fv) / np.sqrt(np.float64(Ee) * np.float64(Et)))
    return {"u": u, "tau": (dstar + fk / F) + delta, "rho": rho, "E_t": float(Et), "v_peak": fv, "d_int": dstar, "flags": flags,
            "z": z, "k": fk, "E_e": float(Ee), "delta": delta, "fine": fine}


def drift_lag_sum(e, tb, x0):
    """sum_i e[x0 + i] tb[i] over the block tb, samples of e outside the clip being zeros: exactly rounded"""
    lo, hi = max(0, -x0), min(len(tb), len(e) - x0)
    return _fsum((e[x0 + lo:x0 + hi] * tb[lo:hi]).tolist()) if hi > lo else 0.0


def _drift_moment(tb):
    """(sum t^2, sum i t^2) of a block, both exactly rounded: a square of a float32 value has 48 bits and is split into two
    halves whose products with i are exact"""
    sq = tb * tb
    hi = sq.astype(np.float32).astype(np.float64)
    i = np.arange(len(tb), dtype=np.float64)
    return _fsum(sq.tolist()), _fsum((i * hi).tolist() + (i * (sq - hi)).tolist())


def drift_reference(e, t, ca=0.0, cb=0.0, radius=64, corr=False, table=None):
    """The segments of estimate e against target t (float32 values) tracked around the centre line (ca, cb) within `radius`
    lags, as the header defines them -> one dict per segment by DRIFT_FIELDS (plus k, E_e, delta and the fine values, for
    the tests).  Every sum over samples is exactly rounded.  corr=True: plus "corr", the lag vector float64 [2 (R + T) + 1].
    table: (G, D), by default the numpy design."""
    R, T, B, H = int(radius), DRIFT_T, DRIFT_BLOCK, DRIFT_HOP
    if not 1 <= R <= DRIFT_MAX_RADIUS:
        raise ValueError("drift_reference: radius 1 ... %d" % DRIFT_MAX_RADIUS)
    _drift_line_check("drift_reference", ca, cb)
    G = (table or drift_table())[0]
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    t = np.asarray(t, dtype=np.float32).astype(np.float64)
    out = []
    for j, z in enumerate(drift_centres(ca, cb, drift_segments(len(t)))):
        tb = t[j * H:j * H + B]
        c = np.array([drift_lag_sum(e, tb, j * H + d) for d in range(z - R - T, z + R + T + 1)])
        Et, N = _drift_moment(tb)

        def Ee_of(d, j=j):
            lo, hi = max(0, j * H + d), min(len(e), j * H + d + B)
            return _fsum((e[lo:hi] ** 2).tolist()) if hi > lo else 0.0

        rec = drift_peak(c, R, z, Et, Ee_of, j * H, N, G)
        if corr:
            rec["corr"] = c
        out.append(rec)
    return out


def drift_fit(records, rho_min=DRIFT_RHO_MIN, trim=DRIFT_TRIM):
    """nhans_drift_fit restated: records (dicts by DRIFT_FIELDS, or rows of NHANS_DRIFT_FIELDS doubles) of one clip -> dict
    by DRIFT_FIT_FIELDS.  Plain Python floats: every operation below is one rounded double operation, in the library's order."""
    rows = [[float(r[k]) for k in DRIFT_FIELDS] if isinstance(r, dict) else [float(v) for v in r] for r in records]
    use = [r for r in rows if r[6] == 0.0 and r[2] >= rho_min]
    n_valid = len(use)
    nan = float("nan")

    def fit(use):
        W = su = st = 0.0
        for r in use:
            W = W + r[3]
            su = su + r[3] * r[0]
            st = st + r[3] * r[1]
        if not W > 0.0:
            return None
        mu, mt = su / W, st / W
        Suu = Sut = 0.0
        for r in use:
            du, dt = r[0] - mu, r[1] - mt
            wdu = r[3] * du
            Suu = Suu + wdu * du
            Sut = Sut + wdu * dt
        if not Suu > 0.0:
            return None
        b = Sut / Suu
        return mt - b * mu, b

    res = lambda r, f: r[1] - (f[0] + f[1] * r[0])
    f = fit(use)
    if f is not None:
        kept = [r for r in use if abs(res(r, f)) <= trim]
        if len(kept) != len(use):
            use = kept
            f = fit(use)
    rms = nan
    if f is not None:
        W = S = 0.0
        for r in use:
            e = res(r, f)
            W = W + r[3]
            S = S + (r[3] * e) * e
        rms = math.sqrt(S / W)
    a, b = f if f is not None else (nan, nan)
    ok = f is not None and len(use) >= 3 and abs(b) <= DRIFT_MAX_SLOPE
    return {"a": a, "b": b, "n_valid": n_valid, "n_used": len(use), "rms_residual": rms, "fit_ok": int(ok)}


def drift_fit_record(values):
    """the NHANS_DRIFT_FIT_FIELDS doubles of nhans_drift_fit -> dict by DRIFT_FIT_FIELDS"""
    return {k: (int(values[i]) if k in ("n_valid", "n_used", "fit_ok") else float(values[i])) for i, k in enumerate(DRIFT_FIT_FIELDS)}


def drift_segment_record(values):
    """the NHANS_DRIFT_FIELDS doubles of one segment -> dict by DRIFT_FIELDS"""
    return {k: (int(values[i]) if k in ("d_int", "flags", "z") else float(values[i])) for i, k in enumerate(DRIFT_FIELDS)}


def drift_warp_reference(e, nt, a, b, table=None):
    """The estimate e (float32 values) resampled at p(u) = a + u + b u for the u of drift_range(len(e), nt, a, b) -> (float32
    [u_hi - u_lo], u_lo, u_hi): the chain of the header, operation by operation -- with the library's own table
    (table=drift_library_table()) what the device gives bit for bit.  table: (G, D), by default the numpy design."""
    T, Q = DRIFT_T, DRIFT_Q
    G, D = table or drift_table()
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    u_lo, u_hi = drift_range(len(e), int(nt), a, b)
    if u_hi == u_lo:
        return np.zeros(0, np.float32), 0, 0
    p = drift_pos(a, b, np.arange(u_lo, u_hi, dtype=np.float64))
    fl = np.floor(p)
    m = fl.astype(np.int64)
    f = (p - fl) * Q
    q = np.minimum(f.astype(np.int64), Q - 1)
    lam = f - q
    acc = np.zeros(len(p))
    for j in range(2 * T):
        x = m + j - (T - 1)
        ok = (x >= 0) & (x < len(e))
        ev = np.where(ok, e[np.clip(x, 0, len(e) - 1)], 0.0)
        acc = _fma(ev, _fma(lam, D[q, j], G[q, j]), acc)
    return acc.astype(np.float32), u_lo, u_hi


def drift_cut(t, u_lo, u_hi):
    """the target (or a signal that is sample-aligned with it) over the range of a warp"""
    return t[u_lo:u_hi]


# ---- LLR, cepstral distance, fwSegSNR: the float64 definition (include/nhans_hip.h: nhans_quality) -------
_quality_tables = None


def _quality_host_tables():
    """(w [480], W [25, 257]): the very tables the library uploads (nhans_quality_tables, host only)."""
    global _quality_tables
    if _quality_tables is None:
        import ctypes
        from . import hip
        w, W = np.zeros(QUALITY_FRAME), np.zeros((QUALITY_BANDS, QUALITY_BINS))
        dp = ctypes.POINTER(ctypes.c_double)
        hip.check(hip.load().nhans_quality_tables(w.ctypes.data_as(dp), W.ctypes.data_as(dp)))
        _quality_tables = (w, W)
    return _quality_tables


def quality_window():
    """w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 481), i < 480: the table the device reads, bit for bit."""
    return _quality_host_tables()[0].copy()


def quality_band_matrix():
    """The default band matrix, float64 [25, 257]: triangles on the HTK mel scale between 0 and 8000 Hz over the bin
    frequencies 31.25 k -- fbank.design's construction on 257 bins, built by the library on the host."""
    return _quality_host_tables()[1].copy()


def quality_num_frames(n):
    return (int(n) - QUALITY_FRAME) // QUALITY_HOP + 1 if n >= QUALITY_FRAME else 0


def quality_frames(x, w):
    """the windowed frames of x (float64), [M, 480]: frame f is x[120 f : 120 f + 480] * w"""
    M = quality_num_frames(len(x))
    idx = QUALITY_HOP * np.arange(M)[:, None] + np.arange(QUALITY_FRAME)[None, :]
    return x[idx] * w[None, :] if M else np.zeros((0, QUALITY_FRAME))


def quality_autocorr(xw):
    """r[0 .. 16] of one windowed frame, every sum exactly rounded"""
    N = len(xw)
    return np.array([_fsum((xw[:N - k] * xw[k:]).tolist()) for k in range(QUALITY_ORDER + 1)])


def _pos_finite(v):
    return v > 0.0 and math.isfinite(v)


def quality_levinson(r):
    """Levinson-Durbin on r[0 .. 16] -> (a [17] with a[0] = 1, [E_1 .. E_16], ok): ok is False where r[0] == 0 or an E_m is
    not a positive finite number (the recursion stops there)."""
    P = QUALITY_ORDER
    a = np.zeros(P + 1)
    a[0] = 1.0
    E, errs = float(r[0]), []
    if r[0] == 0.0:
        return a, errs, False
    for m in range(1, P + 1):
        k = -_fsum([r[m]] + [a[j] * r[m - j] for j in range(1, m)]) / E
        a[1:m] = a[1:m] + k * a[1:m][::-1]
        a[m] = k
        E = E * (1.0 - k * k)
        errs.append(E)
        if not _pos_finite(E):
            return a, errs, False
    return a, errs, True


def quality_toeplitz(r):
    i = np.arange(len(r))
    return np.asarray(r)[np.abs(i[:, None] - i[None, :])]


def quality_form(a, r):
    """a' R a with R[i][j] = r[|i - j|]"""
    return _fsum((a[:, None] * quality_toeplitz(r) * a[None, :]).ravel().tolist())


def quality_cepstrum(a):
    """c[0 .. 16] (c[0] = 0) of the all-pole model 1 / A(z): c[m] = -a[m] - sum_{k < m} (k / m) c[k] a[m - k]"""
    P = QUALITY_ORDER
    c = np.zeros(P + 1)
    for m in range(1, P + 1):
        c[m] = -a[m] - _fsum([(k / m) * c[k] * a[m - k] for k in range(1, m)])
    return c


def quality_lpc_frame(tw, ew):
    """One frame pair (windowed, float64) -> dict: r_t, r_e, a_t, a_e, num, den, dc2, llr, cd (NaN where skipped), ok."""
    rt, re_ = quality_autocorr(tw), quality_autocorr(ew)
    at, _, okt = quality_levinson(rt)
    ae, _, oke = quality_levinson(re_)
    out = {"r_t": rt, "r_e": re_, "a_t": at, "a_e": ae, "num": float("nan"), "den": float("nan"), "dc2": float("nan"),
           "llr": float("nan"), "cd": float("nan"), "ok": False}
    if not (okt and oke):
        return out
    num, den = quality_form(ae, rt), quality_form(at, rt)
    d = quality_cepstrum(at) - quality_cepstrum(ae)
    out.update(num=num, den=den, dc2=_fsum((d[1:] * d[1:]).tolist()))
    if not (_pos_finite(num) and _pos_finite(den)):
        return out
    llr = min(max(math.log(num / den), 0.0), QUALITY_LLR_MAX)
    cd = min(max(QUALITY_CD_SCALE * math.sqrt(2.0 * out["dc2"]), 0.0), QUALITY_CD_MAX)
    out.update(llr=llr + 0.0, cd=cd + 0.0, ok=True)
    return out


def quality_band_sums(fw_frames, W):
    """|rfft(frames, 512)| @ W' with exactly rounded sums -> [M, K]"""
    X = np.abs(np.fft.rfft(fw_frames, n=QUALITY_FFT, axis=1)) if len(fw_frames) else np.zeros((0, QUALITY_BINS))
    return np.array([[_fsum((w * x).tolist()) for w in W] for x in X], dtype=np.float64).reshape(len(X), len(W))


def quality_fw_frame(X, Y):
    """The frequency-weighted segmental SNR of one frame from its band sums X (target) and Y (estimate): 35 less the
    weighted mean of the bands' deficits 35 - s_j; NaN where the weights sum to zero."""
    s = []
    for x, y in zip(X, Y):
        if x == y:
            s.append(QUALITY_SNR_MAX)
        else:
            s.append(min(max(_db(_div(x * x, (x - y) * (x - y))), QUALITY_SNR_MIN), QUALITY_SNR_MAX))
    g = [float(x) ** QUALITY_GAMMA for x in X]
    G = _fsum(g)
    return QUALITY_SNR_MAX - _fsum([a * (QUALITY_SNR_MAX - b) for a, b in zip(g, s)]) / G if G != 0.0 else float("nan")


def quality_trimmed_mean(values):
    """The mean of the q = (19 Mk + 10) // 20 smallest of the Mk values (NaN for none)."""
    v = sorted(values)
    q = (19 * len(v) + 10) // 20
    return _fsum(v[:q]) / q if q else float("nan")


def quality_summary(n, per):
    """The record of a clip of n common samples from its per-frame values [frames, 3] (NaN: skipped) -> dict by
    QUALITY_FIELDS."""
    llr, cd, fw = ([float(v) for v in per[:, k] if v == v] for k in range(3))
    mean = lambda v: _fsum(v) / len(v) if v else float("nan")
    return {"n": int(n), "frames": len(per), "frames_lpc": len(llr), "frames_fw": len(fw), "llr": mean(llr),
            "llr_95": quality_trimmed_mean(llr), "cd_db": mean(cd), "cd_95_db": quality_trimmed_mean(cd), "fwsegsnr_db": mean(fw)}


def quality_reference(e, t, per_frame=False, bands=None, details=False):
    """LLR, cepstral distance and frequency-weighted segmental SNR of estimate e against target t (float32 values at 16 kHz;
    scored over the common prefix) as the header defines them -> dict by QUALITY_FIELDS.  per_frame=True: plus "per_frame",
    float64 [frames, 3] = llr_f, cd_f, fw_f, NaN where the frame was skipped.  bands: a non-negative [K <= 32, 257] matrix
    (None: quality_band_matrix()).  details=True: plus "lpc", one quality_lpc_frame dict per frame, and "band_sums",
    (X, Y) float64 [frames, K]."""
    n = min(len(e), len(t))
    e = np.asarray(e[:n], dtype=np.float32).astype(np.float64)
    t = np.asarray(t[:n], dtype=np.float32).astype(np.float64)
    W = quality_band_matrix() if bands is None else np.asarray(bands, dtype=np.float64)
    if W.ndim != 2 or W.shape[1] != QUALITY_BINS or not 1 <= W.shape[0] <= QUALITY_MAX_BANDS or not (W >= 0).all() \
            or not np.isfinite(W).all():
        raise ValueError("quality_reference: bands is a non-negative finite [K <= %d, %d] matrix" % (QUALITY_MAX_BANDS, QUALITY_BINS))
    w = quality_window()
    ft, fe = quality_frames(t, w), quality_frames(e, w)
    M = len(ft)
    lpc = [quality_lpc_frame(ft[f], fe[f]) for f in range(M)]
    X, Y = quality_band_sums(ft, W), quality_band_sums(fe, W)
    per = np.array([[lpc[f]["llr"], lpc[f]["cd"], quality_fw_frame(X[f], Y[f])] for f in range(M)], dtype=np.float64).reshape(M, 3)
    out = quality_summary(n, per)
    if per_frame:
        out["per_frame"] = per
    if details:
        out.update(lpc=lpc, band_sums=(X, Y))
    return out
