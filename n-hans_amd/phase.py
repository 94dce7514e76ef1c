"""Phase refinement in float64 numpy: the definition of include/nhans_hip.h (nhans_phase_*), operation by operation.

A clip has T frames of 201 bins.  A = exp(lm).  u(z) = z / |z|, and 1 + 0j where |z| is zero or below the smallest normal
float32.  One projection P(lm, t): c = A u(t); x = inverse 400-point real transform of every frame of c (the imaginary
parts of bins 0 and 200 do not enter), synthesis window, overlap-add at hop 160; d = analysis window and forward transform
of the frames of x.  Griffin-Lim with momentum alpha: t_0 = exp(i ph), d_n = P(lm, t_n), t_{n+1} = d_n + alpha (d_n -
d_{n-1}) with d_{-1} := d_0; after N iterations the phases are angle(t_N), the waveform is the inverse transform of
A exp(i angle(t_N)), and inc[n] = sum (|d_n| - A)^2 / sum A^2.

The module stands alone (numpy only): it is what the device results are held to, and what a reader checks the header
against.  The clip edges are not perfect-reconstruction regions of the window pair, so P is not idempotent there and inc
need not fall monotonically.
"""
import numpy as np

WIN, HOP, BINS = 400, 160, 201
MAX_ITERS = 256
RUN = 20                    # frames per run of the projection kernel (kPhaseRun)
SMALLEST_NORMAL = float(np.finfo(np.float32).tiny)


def analysis_window():
    """The periodic Hann window of the analysis transform."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN, dtype=np.float64) / WIN)


def synthesis_window():
    """w[n] / sum_q w^2[n mod 160 + 160 q]: the window under which overlap-add at hop 160 undoes the analysis window."""
    w = analysis_window()
    den = np.zeros(HOP)
    for q in range(-(-WIN // HOP)):
        seg = w[q * HOP:(q + 1) * HOP] ** 2
        den[:len(seg)] += seg
    return w / np.tile(den, -(-WIN // HOP))[:WIN]


def unit(z):
    """z / |z|; 1 + 0j where |z| is zero or below the smallest normal float32."""
    z = np.asarray(z, dtype=np.complex128)
    m = np.abs(z)
    small = m < SMALLEST_NORMAL
    return np.where(small, 1.0 + 0.0j, z / np.where(small, 1.0, m))


def synthesise(c):
    """complex [T, 201] -> the (T - 1) 160 + 400 samples: inverse transform, synthesis window, overlap-add."""
    c = np.asarray(c, dtype=np.complex128)
    t = c.shape[0]
    if t == 0:
        return np.zeros(0)
    frames = np.fft.irfft(c, n=WIN, axis=1) * synthesis_window()[None, :]
    out = np.zeros((t - 1) * HOP + WIN)
    for i in range(t):
        out[i * HOP:i * HOP + WIN] += frames[i]
    return out


def analyse(x):
    """samples -> complex [T, 201]: analysis window and forward transform of every whole frame."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) < WIN:
        return np.zeros((0, BINS), dtype=np.complex128)
    t = 1 + (len(x) - WIN) // HOP
    idx = np.arange(WIN)[None, :] + HOP * np.arange(t)[:, None]
    return np.fft.rfft(x[idx] * analysis_window()[None, :], n=WIN, axis=1)


def project_reference(lm, t):
    """P(lm, t): lm real [T, 201], t complex [T, 201] -> d complex128 [T, 201]."""
    a = np.exp(np.asarray(lm, dtype=np.float64))
    return analyse(synthesise(a * unit(t)))


def inconsistency(lm, d):
    """sum (|d| - A)^2 / sum A^2 of one clip."""
    a = np.exp(np.asarray(lm, dtype=np.float64))
    return float(((np.abs(d) - a) ** 2).sum() / (a ** 2).sum())


def reference(lm, ph, iters, alpha=0.0, states=False):
    """N = iters Griffin-Lim iterations on one clip from the phases ph -> dict(phase [T, 201], inc [N], wave); with
    states=True also t = [t_0 ... t_N] and d = [d_0 ... d_{N-1}] (complex128).  iters = 0 returns ph itself."""
    if not 0 <= iters <= MAX_ITERS:
        raise ValueError("iters must be in [0, %d], not %r" % (MAX_ITERS, iters))
    if not 0.0 <= alpha < 1.0:
        raise ValueError("alpha must be in [0, 1), not %r" % (alpha,))
    lm = np.asarray(lm, dtype=np.float64)
    ph = np.asarray(ph)
    t = np.exp(1j * ph.astype(np.float64))
    ts, ds, inc = [t], [], []
    prev = None
    for _ in range(iters):
        d = project_reference(lm, t)
        t = d + alpha * (d - (d if prev is None else prev))
        prev = d
        ts.append(t)
        ds.append(d)
        inc.append(inconsistency(lm, d))
    phase = ph if iters == 0 else np.angle(t)
    out = {"phase": phase, "inc": np.array(inc, dtype=np.float64),
           "wave": synthesise(np.exp(lm) * np.exp(1j * np.asarray(phase, dtype=np.float64)))}
    if states:
        out["t"], out["d"] = ts, ds
    return out


def si_sdr(est, tgt):
    """Scale-invariant SDR in dB of est against tgt over their common prefix (float64; no mean removal)."""
    n = min(len(est), len(tgt))
    e, s = np.asarray(est[:n], dtype=np.float64), np.asarray(tgt[:n], dtype=np.float64)
    p = (e @ s) / (s @ s) * s
    return float(10.0 * np.log10((p @ p) / ((e - p) @ (e - p))))
