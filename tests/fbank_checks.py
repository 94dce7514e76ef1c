"""What tests/test_fbank_host.py and tests/test_gpu_fbank.py share: the numpy restatement of the triangular designer
(include/nhans_hip.h: nhans_fbank_design), the input domain and its batch, the parity banks and the float64 bar.

The bar.  out[m] = logf(max(sum_k w p, floor)) with the sum one float32 fmaf chain over the band's K_m bins: one rounding
per tap (every term is non-negative, so K_m roundings of relative size 2^-24 move ln of the sum by at most K_m 2^-24),
one ulp-class error each of expf (relative in p, hence absolute in ln) and logf, and the half-ulp of the stored result,
2^-24 |ref|.  Hence err <= c 2^-24 (K_m + |ref| + 1) for a small c.  C_BAR is the smallest power of two that is at least
twice the worst err / (2^-24 (K_m + |ref| + 1)) measured on the device against the float64 reference over the whole
parity batch of tests/test_gpu_fbank.py (profiles/fbank/README.md has the measurement); the factor two is for devices
and compilers not met.  The condition set with the bar is C_BAR <= 16; a ratio above 8 would be a defect to find."""
import math

import numpy as np

from nhans_amd import fbank, spec

TILE = 16                                   # rows per workgroup of fbank.hip (kFbankTile)
C_BAR = 8.0
LO, HI = math.log(1e-5) - 20.0, 16.0        # the domain of the network's rows (nhans_istft's header comment)
EPS = 2.0 ** -24


# ---- the designer, restated -----------------------------------------------------------------------
def hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)))


def np_design(n, f_min, f_max, scale, norm):
    """-> (W float64 [n, 201], the n + 2 edge frequencies, the triangles' peak heights [n])."""
    m0, m1 = float(hz_to_mel(f_min, scale)), float(hz_to_mel(f_max, scale))
    p = mel_to_hz(m0 + (m1 - m0) * np.arange(n + 2, dtype=np.float64) / float(n + 1), scale)
    f = 40.0 * np.arange(spec.BINS, dtype=np.float64)
    up = (f[None, :] - p[:-2, None]) / (p[1:-1] - p[:-2])[:, None]
    down = (p[2:, None] - f[None, :]) / (p[2:] - p[1:-1])[:, None]
    W = np.maximum(0.0, np.minimum(up, down))
    peak = np.ones(n)
    if norm == "slaney":
        peak = 2.0 / (p[2:] - p[:-2])
        W = W * peak[:, None]
    return W, p, peak


def empty_bands(W):
    return int((~(W.astype(np.float32) != 0).any(axis=1)).sum())


# ---- banks and rows -------------------------------------------------------------------------------
def custom_matrix():
    """An all-ones band (201 taps: the longest chain), a single-tap band, an empty band and a two-tap band with a gap."""
    W = np.zeros((4, spec.BINS))
    W[0, :] = 1.0
    W[1, 117] = 0.75
    W[3, 5], W[3, 9] = 0.5, 1.5
    return W


_banks = {}


def bank(name):
    if name not in _banks:
        _banks[name] = {
            "htk80": lambda: fbank.Filterbank(80, scale="htk", power=2),
            "slaney128": lambda: fbank.Filterbank(128, scale="slaney", norm="slaney", power=2),
            "htk40p1": lambda: fbank.Filterbank(40, scale="htk", power=1),
            "custom": lambda: fbank.Filterbank.from_matrix(custom_matrix(), power=2, floor=1e-10),
        }[name]()
    return _banks[name]


BANKS = ["htk80", "slaney128", "htk40p1", "custom"]


def uniform_rows(n, seed=5):
    return np.random.default_rng(seed).uniform(LO, HI, size=(n, spec.BINS)).astype(np.float32)


def edge_rows():
    """all-minimum, all-maximum, and for every bin: that bin at the maximum, the rest at the minimum"""
    lo, hi = np.float32(LO), np.float32(HI)
    one = np.full((spec.BINS, spec.BINS), lo, dtype=np.float32)
    one[np.arange(spec.BINS), np.arange(spec.BINS)] = hi
    return np.concatenate([np.full((1, spec.BINS), lo, np.float32), np.full((1, spec.BINS), hi, np.float32), one])


def ratio(fb, got, ref):
    """err / (2^-24 (K_m + |ref| + 1)) per element"""
    K = fb.spans()[1].astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / (EPS * (K[None, :] + np.abs(ref) + 1.0))


def bar(fb, ref):
    K = fb.spans()[1].astype(np.float64)
    return C_BAR * EPS * (K[None, :] + np.abs(ref) + 1.0)


def shifted(fb):
    """The same bank one bin too high: the fault a misplaced edge or an off-by-one span makes."""
    W = np.zeros_like(fb.matrix)
    W[:, 1:] = fb.matrix[:, :-1]
    return fbank.Filterbank.from_matrix(W, fb.power, fb.floor)
