"""What the full-band tests share (include/nhans_hip.h: nhans_fullband_*): the hold bound by brute force over
live.emitted, and the definition restated in numpy -- in float64 with scipy's resample_poly, and in float32 with the
operations of the header one numpy operation each."""
import numpy as np

import nhans_amd  # noqa: F401
from nhans_amd import hip, live, resample

RATES = hip.FULLBAND_RATES
HOP = 160


def scan_limit(rate):
    """Input samples after which N - emitted(N) only repeats: the first pair of hops is out once 19 frames exist at
    16 kHz (3,280 samples, 0.205 s) plus the two filters' delay (under 2 ms), and from then on 20 ms of input -- rate / 50
    samples, 320 at 16 kHz, one pair of hops -- bring rate / 50 outputs.  0.3 s holds the start and three periods."""
    return int(0.3 * rate)


def hold_brute(rate, lookaheads=range(18)):
    """max over N and L of N - live.emitted(N, False, rate, rate, L): the header's H(rate)."""
    best = 0
    for L in lookaheads:
        for n in range(scan_limit(rate) + 1):
            best = max(best, n - live.emitted(n, False, rate, rate, L))
    return best


def ratio(rate):
    from math import gcd
    g = gcd(rate, 16000)
    return rate // g, 16000 // g          # (up, down) of 16 kHz -> rate


def round_trip64(u, rate):
    """R(R_in(u)) in float64: rate -> 16 kHz -> rate with resample_poly's default filter, cut to len(u)."""
    from scipy.signal import resample_poly
    up, down = ratio(rate)
    back = resample_poly(resample_poly(np.asarray(u, np.float64), down, up), up, down)
    out = np.zeros(len(u))
    n = min(len(u), len(back))
    out[:n] = back[:n]
    return out


def combined(den, mix, wet):
    """c = den + (mix - den) * w in float32, three numpy operations; wet a scalar or one factor per hop."""
    if np.ndim(wet):
        w = np.repeat(np.asarray(wet, dtype=np.float32), HOP)[:len(den)]
        assert len(w) == len(den)
    else:
        if float(wet) == 0.0:
            return den.copy()
        w = np.float32(wet)
    c = den + (mix - den) * w
    assert c.dtype == np.float32
    return c


def u_of(x, in_denom, n):
    """u[0 .. n): float32(double(x) / in_denom), 0 past the end of x."""
    u = np.zeros(n, np.float32)
    k = min(n, len(x))
    u[:k] = (np.asarray(x[:k], np.float32).astype(np.float64) / in_denom).astype(np.float32)
    return u


def restate64(x, den, mix, rate, in_denom, wet, g):
    """y before the sink, in float64 from the float32 inputs: R(c - g m) + g x / in_denom, g the float32 gain."""
    from scipy.signal import resample_poly
    up, down = ratio(rate)
    g = float(np.float32(g))
    d, m = den.astype(np.float64), mix.astype(np.float64)
    if np.ndim(wet):
        w = np.repeat(np.asarray(wet, np.float32).astype(np.float64), HOP)[:len(den)]
    else:
        w = float(np.float32(wet))
    e = d + (m - d) * w - g * m
    lo = resample_poly(e, up, down)
    assert len(lo) == resample.out_count(len(den), 16000, rate)
    u = np.zeros(len(lo))
    k = min(len(lo), len(x))
    u[:k] = np.asarray(x[:k], np.float32).astype(np.float64) / in_denom
    return lo + g * u


def residual32(den, mix, wet, g):
    """e = c - g * m in float32: the product and the difference rounded separately."""
    e = combined(den, mix, wet) - np.float32(g) * mix
    assert e.dtype == np.float32
    return e


def add_high32(lo, x, in_denom, g):
    """y = lo + g * u in float32, two operations."""
    y = lo + np.float32(g) * u_of(x, in_denom, len(lo))
    assert y.dtype == np.float32
    return y


def pcm(y, out_dtype, scale):
    """The outgoing sink: float32(double(y) * scale), rounded and clipped for int16."""
    v = (y.astype(np.float64) * scale).astype(np.float32)
    if np.dtype(out_dtype) == np.float32:
        return v
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def tone(rate, hz, seconds=0.25):
    return np.sin(2 * np.pi * hz * np.arange(int(seconds * rate)) / rate)


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def cpu32(x, rate):
    """The float32 restatement of the 16 kHz -> rate conversion on the CPU: taps rounded to float32, one sequential
    float32 accumulation per output (multiply, round, add, round), taps in the kernel's order."""
    pair = (16000, rate)
    L, M, half, J = resample.geometry(*pair)
    h = np.zeros(L * J, np.float32)
    t = resample.taps(*pair).astype(np.float32)
    h[:len(t)] = t
    n = len(x)
    m = np.arange(resample.out_count(n, *pair), dtype=np.int64)
    q, p = np.divmod(m * M + half, L)
    xp = np.concatenate([np.zeros(J, np.float32), np.asarray(x, np.float32), np.zeros(J + half // L + 2, np.float32)])
    acc = np.zeros(len(m), np.float32)
    for j in range(J):
        k = q - j
        xv = np.where((k >= 0) & (k < n), xp[np.clip(k, -J, n + J) + J], np.float32(0))
        acc = (h[p + j * L] * xv).astype(np.float32) + acc
    return acc
