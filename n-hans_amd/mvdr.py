"""Mask-driven MVDR beamforming in float64 numpy: the definition of include/nhans_hip.h (nhans_mvdr_*), operation by
operation.

A clip has C channels of n samples, x [n, C], and T frames.  X_c = the analysis transform of channel c (phase.analyse:
what nhans_stft_features holds before its log and angle).  A mask m [T, 201] in [0, 1] (a NaN counts as 0; a log-gain g
gives m = min(1, exp(g))) weighs the frames of two covariances per bin, Phi_s = sum_t m x x^H and Phi_n = sum_t (1 - m)
x x^H.  Phi_n' = Phi_n + loading (tr Phi_n / C) I = L L^H (Cholesky), G = Phi_n'^-1 Phi_s by two triangular solves per
column, tau = Re tr G, w = G[:, ref] / tau: Souden's form of the MVDR filter -- no steering vector, no
eigen-decomposition, unchanged when either mask's sum is scaled.  Where tr Phi_n = 0, a pivot is not positive and finite,
tau is not positive and finite or w is not finite, w = e_ref: the reference channel passes through and the bin counts in
fallback_bins.  y = w^H x, and the output is rows: log(max(|y|, 1e-5)) and angle(y).

The module stands alone (numpy only): it is what the device results are held to, and what a reader checks the header
against.  Every stage takes its input as an argument, so a test can hand it the device's own output of the stage before.
"""
import numpy as np

from . import phase as phase_mod

WIN, HOP, BINS = phase_mod.WIN, phase_mod.HOP, phase_mod.BINS
MAX_CHANNELS = 8
LOADING = 1e-6
FLOOR = 1e-5
FIELDS = ("frames", "channels", "ref", "fallback_bins", "energy_ref", "energy_out")


def check(channels, ref, loading):
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("1 ... %d channels, not %r" % (MAX_CHANNELS, channels))
    if not 0 <= ref < channels:
        raise ValueError("ref must be in [0, %d), not %r" % (channels, ref))
    if not 0.0 <= loading <= 1.0:
        raise ValueError("loading must be in [0, 1], not %r" % (loading,))


def planes(x):
    """[n, C] samples, as a sound-file reader hands them over -> the C planes one after the other (float32, flat)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("a clip is an [n, C] array")
    return np.ascontiguousarray(x.T).reshape(-1)


def spectra(x):
    """[n, C] samples -> X complex128 [C, T, 201]."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([phase_mod.analyse(x[:, c]) for c in range(x.shape[1])])


def mask_values(rows, loggain=False):
    """Mask rows (or, loggain: log-gain rows) [T, 201] -> m in [0, 1], float64; a NaN counts as 0."""
    v = np.asarray(rows, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if loggain:
            v = np.where(v > 0.0, 1.0, np.exp(np.minimum(v, 0.0)))
        return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 1.0))


def covariances(X, m):
    """X complex [C, T, 201], m [T, 201] -> (Phi_s, Phi_n) complex128 [201, C, C], the frames summed in ascending order."""
    X = np.asarray(X, dtype=np.complex128)
    m = np.asarray(m, dtype=np.float64)
    C, T, K = X.shape
    ps, pn = np.zeros((K, C, C), np.complex128), np.zeros((K, C, C), np.complex128)
    for t in range(T):
        x = X[:, t, :].T                                    # [K, C]
        p = x[:, :, None] * np.conj(x[:, None, :])          # x x^H
        ps += m[t][:, None, None] * p
        pn += (1.0 - m[t])[:, None, None] * p
    return ps, pn


def weights(phi_s, phi_n, ref=0, loading=LOADING, dtype=np.complex128):
    """(Phi_s, Phi_n) [K, C, C] -> (w [K, C], fallback [K] bool).  dtype: the arithmetic (np.clongdouble gives a teacher of
    higher precision for the tests' bars)."""
    cdt = np.dtype(dtype)
    rdt = np.empty(0, cdt).real.dtype
    S, A = np.array(phi_s, dtype=cdt), np.array(phi_n, dtype=cdt)
    K, C, _ = A.shape
    check(C, ref, loading)
    with np.errstate(all="ignore"):
        tr = np.zeros(K, rdt)
        for i in range(C):
            tr = tr + A[:, i, i].real
        ok = tr != 0
        add = rdt.type(loading) * (tr / rdt.type(C))
        for i in range(C):
            A[:, i, i] = A[:, i, i] + add
        L = np.zeros((K, C, C), cdt)
        for j in range(C):
            d = A[:, j, j].real.copy()
            for q in range(j):
                d = d - (L[:, j, q].real ** 2 + L[:, j, q].imag ** 2)
            ok &= (d > 0) & np.isfinite(d)
            ljj = np.sqrt(d)
            L[:, j, j] = ljj
            for i in range(j + 1, C):
                s = A[:, i, j].copy()
                for q in range(j):
                    s = s - L[:, i, q] * np.conj(L[:, j, q])
                L[:, i, j] = s / ljj
        tau = np.zeros(K, rdt)
        g_ref = np.zeros((K, C), cdt)
        for col in range(C):
            g = np.zeros((K, C), cdt)
            for i in range(C):                              # L y = b
                s = S[:, i, col].copy()
                for q in range(i):
                    s = s - L[:, i, q] * g[:, q]
                g[:, i] = s / L[:, i, i].real
            for i in range(C - 1, -1, -1):                  # L^H g = y
                s = g[:, i].copy()
                for q in range(C - 1, i, -1):
                    s = s - np.conj(L[:, q, i]) * g[:, q]
                g[:, i] = s / L[:, i, i].real
            tau = tau + g[:, col].real
            if col == ref:
                g_ref = g
        ok &= (tau > 0) & np.isfinite(tau)
        w = g_ref / tau[:, None]
        ok &= np.isfinite(w.real).all(axis=1) & np.isfinite(w.imag).all(axis=1)
    e = np.zeros((K, C), cdt)
    e[:, ref] = 1
    return np.where(ok[:, None], w, e), ~ok


def apply(X, w):
    """X complex [C, T, 201], w complex [201, C] -> y [T, 201] = sum_c conj(w_c) X_c."""
    X, w = np.asarray(X, dtype=np.complex128), np.asarray(w, dtype=np.complex128)
    y = np.zeros(X.shape[1:], np.complex128)
    for c in range(X.shape[0]):
        y = y + np.conj(w[:, c])[None, :] * X[c]
    return y


def rows(y, gain=None):
    """y complex [T, 201] -> (log(max(|y|, 1e-5)) (+ gain), angle(y))."""
    lm = np.log(np.maximum(np.abs(y), FLOOR))
    if gain is not None:
        lm = lm + np.asarray(gain, dtype=np.float64)
    return lm, np.angle(y)


def reference(x, mask, ref=0, loading=LOADING, loggain=False, gain=None, X=None):
    """One clip, x [n, C] and mask rows [T, 201] -> dict(X, m, phi_s, phi_n, w, fallback, y, logmag, phase, record).  X: the
    spectra to use instead of x's own (the device's, say)."""
    X = spectra(x) if X is None else np.asarray(X, dtype=np.complex128)
    C, T, _ = X.shape
    check(C, ref, loading)
    m = mask_values(mask, loggain)
    if m.shape != (T, BINS):
        raise ValueError("the mask is [%d, %d] rows" % (T, BINS))
    ps, pn = covariances(X, m)
    w, fb = weights(ps, pn, ref, loading)
    y = apply(X, w)
    lm, ph = rows(y, gain)
    rec = dict(zip(FIELDS, (float(T), float(C), float(ref), float(fb.sum()), float((np.abs(X[ref]) ** 2).sum()),
                            float((np.abs(y) ** 2).sum()))))
    return {"X": X, "m": m, "phi_s": ps, "phi_n": pn, "w": w, "fallback": fb, "y": y, "logmag": lm, "phase": ph, "record": rec}


def synthesise(y):
    """y complex [T, 201] -> the waveform (phase.synthesise: the library's inverse transform, synthesis window, overlap-add)."""
    return phase_mod.synthesise(y)


def record(values):
    """NHANS_MVDR_FIELDS doubles -> dict by FIELDS."""
    return dict(zip(FIELDS, (float(v) for v in values)))
