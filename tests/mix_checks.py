"""The mixing rule of include/nhans_hip.h (nhans_mix) restated with every dtype explicit, so that the tests of the host
rule (tests/test_mix_host.py) and of the device (tests/test_gpu_mix.py) do not rest on NumPy's promotion rules: every
array operation below has float32 operands of one kind, every scalar one is a Python float (an IEEE double) or an
np.float32, and the chain of the power is a Python loop.  `fault=` plants one wrong reading of the rule at a time; the
tests show that the bit-for-bit comparison sees each."""
import math

import numpy as np

F32 = np.float32
EPS = F32(0.000001)
FIELDS = ("P_s", "P_keep", "P_drop", "g_keep", "g_drop", "pk", "unit")
OUTPUTS = ("mixture", "target", "keep", "drop")
FAULTS = ("pairwise_power", "gain_in_double", "target_by_p", "fit_restarts_per_tile")


def fit(x, n, restart=None):
    """A[i] = x[i mod m] where m < n, else x[i] (restart: the planted fault -- the noise begins again at every tile)."""
    m = len(x)
    i = np.arange(n, dtype=np.int64)
    if restart:
        i = i % restart
    return x[i % m] if m < n else x[i]


def power(x, pairwise=False):
    """float32 squares, added one after the other in float64 from 0.0 on, divided by the count."""
    sq = np.abs(x) * np.abs(x)
    assert sq.dtype == np.float32
    if pairwise:
        return float(np.sum(sq.astype(np.float64))) / float(len(x))
    S = 0.0
    for v in sq.tolist():           # (Python floats: the float32 values, exactly)
        S = S + v
    return S / float(len(x))


def snr_factor(snr_db):
    return pow(10.0, -snr_db / 10.0)


def gain(p_speech, p_noise, snr_db):
    if p_noise == 0.0:
        return 1.0
    return math.sqrt((p_speech / p_noise) * snr_factor(snr_db))


def reference(s, a, b, snr_keep_db, snr_drop_db, fault=None, tile=2048):
    """-> dict: the four float32 outputs (OUTPUTS) and the record's fields (FIELDS, Python floats).  a = None: the
    two-way mix (target = s / unit, keep = zeros)."""
    assert fault is None or fault in FAULTS
    s = np.ascontiguousarray(s, dtype=F32)
    n = len(s)
    restart = tile if fault == "fit_restarts_per_tile" else None
    pw = fault == "pairwise_power"
    B = fit(np.asarray(b, dtype=F32), n, restart)
    Ps, Pb = power(s, pw), power(B, pw)
    gb = gain(Ps, Pb, snr_drop_db)
    if a is not None:
        A = fit(np.asarray(a, dtype=F32), n, restart)
        Pa = power(A, pw)
        ga = gain(Ps, Pa, snr_keep_db)
        kept = F32(ga) * A
        if fault == "gain_in_double":
            kept = (ga * A.astype(np.float64)).astype(F32)
        wanted = s + kept
    else:
        Pa, ga, kept, wanted = 0.0, 1.0, np.zeros(n, F32), s
    dropped = F32(gb) * B
    if fault == "gain_in_double":
        dropped = (gb * B.astype(np.float64)).astype(F32)
    raw = wanted + dropped
    assert raw.dtype == np.float32 and kept.dtype == np.float32 and dropped.dtype == np.float32
    pk = F32(np.max(np.abs(raw)))
    p = F32(pk + EPS)
    unit = F32(F32(pk / p) + EPS)
    d = p if fault == "target_by_p" else unit
    out = {"mixture": raw / p, "target": wanted / d, "keep": kept / d if a is not None else kept, "drop": dropped / d,
           "P_s": Ps, "P_keep": Pa, "P_drop": Pb, "g_keep": ga, "g_drop": gb, "pk": float(pk), "unit": float(unit)}
    assert all(out[k].dtype == np.float32 for k in OUTPUTS)
    return out


def achieved_snr_db(s, g, noise_fitted):
    """10 log10(sum s^2 / sum (g32 A)^2) in float64 (math.fsum: exact sums)."""
    s64 = np.asarray(s, dtype=F32).astype(np.float64)
    k64 = (F32(g) * np.asarray(noise_fitted, dtype=F32)).astype(np.float64)
    return 10.0 * math.log10(math.fsum(s64 * s64) / math.fsum(k64 * k64))


def signal(n, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def host_cases(lengths=(1, 2, 399, 400, 32400)):
    """(name, s, a, b, snr_keep, snr_drop, plain) for the host rule's lengths: noises shorter (m = 1 and m = n - 1
    included), equal and longer, a silent noise, silent speech; plain: neither silent nor a single sample."""
    out = []
    for n in lengths:
        s = signal(n, 100 + n)
        shorter = sorted({m for m in (1, 7, n // 3, n - 1) if 1 <= m < n})
        for j, m in enumerate(shorter + [n, n + 5, 2 * n + 1]):
            a, b = signal(m, 200 + n + j, 0.1), signal(max(1, (m * 5) // 7 + 1), 300 + n + j, 0.7)
            out.append(("n%d_m%d" % (n, m), s, a, b, (-3, 5)[j % 2], (8, 0, -3)[j % 3], n > 1))
        out.append(("n%d_silent_keep" % n, s, np.zeros(max(1, n // 2), F32), signal(n + 3, 400 + n), 3, -3, False))
        out.append(("n%d_silent_drop" % n, s, signal(n, 500 + n), np.zeros(n + 1, F32), 0, 5, False))
        out.append(("n%d_silent_speech" % n, np.zeros(n, F32), signal(n, 600 + n), signal(max(1, n - 1), 700 + n), 5, 8, False))
        out.append(("n%d_all_silent" % n, np.zeros(n, F32), np.zeros(3, F32), np.zeros(n, F32), 0, 0, False))
    return out


def bits(x):
    x = np.asarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x), bits(y))


def ulps64(x, y):
    """How many doubles lie between two positive doubles."""
    return abs(int(np.float64(x).view(np.int64)) - int(np.float64(y).view(np.int64)))
