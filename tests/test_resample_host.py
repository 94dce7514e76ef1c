"""Sample-rate conversion, the parts that need no device: the filter the library designs in C++ against
scipy.signal.firwin (the filter of scipy.signal.resample_poly), and the output-count / streaming contract of
include/nhans_hip.h -- in C and restated in nhans_amd.resample -- against a brute force over its definition."""
import re
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import hip, online, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = [r for r in resample.RATES if r != 16000]
PAIRS = [(r, 16000) for r in OTHER] + [(16000, r) for r in OTHER]
IDS = ["%d-%d" % p for p in PAIRS]


@pytest.fixture(scope="module")
def lib(lib_built):
    return hip.load()


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_taps_are_firwin(lib, pair):
    """Two float64 evaluations of one formula (sinc x Kaiser(5), unit sum, times L): 1e-12 only has to catch a wrong one."""
    from scipy.signal import firwin
    L, M, half, J = resample.geometry(*pair)
    h = resample.taps(*pair)
    ref = firwin(2 * half + 1, 1.0 / max(L, M), window=("kaiser", 5.0)) * L
    assert h.shape == ref.shape
    err = float(np.abs(h - ref).max())
    print("%s: %d taps, max |h - firwin| = %.2e" % (pair, len(h), err))
    assert err <= 1e-12
    assert J == -(-len(h) // L) and 21 <= J <= 121
    assert L * J * 4 <= 53760                               # the largest phase table: 52.5 KB (11.025 kHz in)


def test_taps_room_and_identity(lib):
    assert lib.nhans_resample_taps(48000, 16000, None, 0) == 61
    buf = (hip.ctypes.c_double * 10)()
    assert lib.nhans_resample_taps(48000, 16000, buf, 10) == -1
    assert b"61" in lib.nhans_last_error()
    assert resample.taps(16000, 16000).tolist() == [1.0]
    assert resample.geometry(16000, 16000) == (1, 1, 0, 1)
    assert resample.out_count(123, 16000, 16000) == 123
    assert resample.emitted(123, False, 16000, 16000) == 123


def _brute_emitted(N, L, M, half):
    """Outputs of the whole clip that are final after N inputs: output m is final iff floor((m M + half) / L) <= N - 1.
    (q(m) grows with m, so the final ones are a prefix.)"""
    whole = -(-(N * L) // M)
    m = 0
    while m < whole and (m * M + half) // L <= N - 1:
        m += 1
    return m


@pytest.mark.parametrize("pair", PAIRS + [(16000, 16000)], ids=IDS + ["16000-16000"])
def test_counts_against_brute_force(lib, pair):
    L, M, half, _ = resample.geometry(*pair)
    around = half // L
    Ns = sorted(set(list(range(0, 301)) + list(range(max(0, around - 12), around + 13)) + [4410 - 1, 4410, 4410 + 1]))
    for N in Ns:
        whole = -(-(N * L) // M)
        assert resample.out_count(N, *pair) == whole
        assert lib.nhans_resample_out_count(N, *pair) == whole
        want = _brute_emitted(N, L, M, half)
        assert resample.emitted(N, False, *pair) == want, (pair, N)
        assert lib.nhans_resample_emitted(N, 0, *pair) == want, (pair, N)
        assert resample.emitted(N, True, *pair) == whole
        assert lib.nhans_resample_emitted(N, 1, *pair) == whole
    # emitted never decreases and the look-ahead is what the header says: half / L inputs (rounded up)
    e = [resample.emitted(N, False, *pair) for N in range(0, 2000)]
    assert all(b >= a for a, b in zip(e, e[1:]))
    first = next(N for N, v in enumerate(e) if v > 0)
    assert first == half // L + 1


@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100), (16000, 16001), (7999, 16000), (0, 16000), (16000, -8000),
                                  (8000, 8000)])
def test_unsupported_pair_is_refused_with_both_rates(lib, pair):
    assert lib.nhans_resample_out_count(100, *pair) < 0
    msg = lib.nhans_last_error().decode()
    assert str(pair[0]) in msg and str(pair[1]) in msg
    assert lib.nhans_resample_taps(pair[0], pair[1], None, 0) == -1
    assert lib.nhans_resample_emitted(100, 0, *pair) < 0
    assert not resample.supported(*pair)
    with pytest.raises(ValueError):
        resample.out_count(100, *pair)
    with pytest.raises(ValueError):
        resample.emitted(100, False, *pair)


def test_negative_count_is_refused(lib):
    assert lib.nhans_resample_out_count(-1, 48000, 16000) < 0


def test_header_declares_what_the_binding_exports(lib):
    """Every new name is in the header, in hip.EXPORTS and in the library; the ABI number did not move."""
    text = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    declared = set(re.findall(r"\b(nhans_resampl\w+|nhans_peak_normalise|nhans_channel_mean)\s*\(", text))
    new = {n for n in hip.EXPORTS if n.startswith("nhans_resampl") or n in ("nhans_peak_normalise", "nhans_channel_mean")}
    assert declared == new and {"nhans_resample", "nhans_resampler_push", "nhans_peak_normalise", "nhans_channel_mean"} <= new
    for n in new:
        getattr(lib, n)
    assert lib.nhans_abi_version() == 5
    for name, value in (("NHANS_PCM_INT16", hip.PCM_INT16), ("NHANS_PCM_FLOAT32", hip.PCM_FLOAT32),
                        ("NHANS_RESAMPLE_QUANTISE", hip.RESAMPLE_QUANTISE), ("NHANS_NORMALISE_WRAP_INT16", hip.NORMALISE_WRAP_INT16)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value


def test_latency_terms():
    """10 periods of the lower rate per conversion: 0.625 ms beside 16 kHz, 1.25 ms beside 8 kHz."""
    assert resample.latency_ms(48000, 16000) == pytest.approx(0.625)
    assert resample.latency_ms(16000, 44100) == pytest.approx(0.625)
    assert resample.latency_ms(8000, 16000) == pytest.approx(1.25)
    lo, hi = online.latency_ms()
    lo2, hi2 = online.latency_ms(in_rate=48000, out_rate=48000)
    assert (lo, hi) == (185.0, 205.0)
    assert lo2 - lo == pytest.approx(1.25) and hi2 - hi == pytest.approx(1.25)
