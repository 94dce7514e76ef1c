"""Full-band live output, the part that needs no device (include/nhans_hip.h: nhans_fullband_*): the names, the hold
bound H(r) against a brute force over live.emitted, a simulated hold under random cuttings, what the entry points refuse
before they need a device, and the definition's own numbers -- how much of a tone u - R(R_in(u)) keeps -- in float64."""
import ctypes
import os
import re

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live

import fullband_checks as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nhans_fullband_hold_samples", "nhans_fullband_live_enable", "nhans_fullband_live_set_gain", "nhans_fullband_mix"]


def test_names_and_abi(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t|void) (nhans_fullband_\w+)\(", header, re.M)))
    assert declared == sorted(NAMES) == sorted(n for n in hip.EXPORTS if n.startswith("nhans_fullband_"))
    lib = hip.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.nhans_abi_version() == hip.ABI_VERSION == 5
    assert int(re.search(r"#define NHANS_ABI_VERSION (\d+)", header).group(1)) == 5
    names = list(hip.SIGNATURES)
    assert max(names.index(n) for n in NAMES) < names.index("nhans_profile_json")
    assert len(hip.SIGNATURES["nhans_fullband_mix"][1]) == 18


@pytest.mark.parametrize("rate", F.RATES)
def test_hold_samples_is_the_brute_force(lib_built, rate):
    """H(r) of the library == max over N <= 0.3 s and L = 0 .. 17 of N - live.emitted(N): after the first pair of hops
    N - emitted(N) repeats every 20 ms (fullband_checks.scan_limit), which the last period scanned confirms."""
    H = live.fullband_hold(rate)
    assert H == F.hold_brute(rate)
    period, top = rate // 50, F.scan_limit(rate)
    for L in (0, 17):
        for n in range(top - period, top + 1):
            assert n - live.emitted(n, False, rate, rate, L) == (n - period) - live.emitted(n - period, False, rate, rate, L)
    # the bound is the longest look-ahead's, and it is more than the look-ahead alone: the window and the pair rule too
    assert H == F.hold_brute(rate, [17]) and H > (17 * 160 + 400) * rate // 16000


def test_unsupported_rates(lib_built):
    lib = hip.load()
    for rate in (8000, 16000, 11025, 44000, 0, -1):
        assert lib.nhans_fullband_hold_samples(rate) == -1
        assert b"nhans_fullband_hold_samples" in lib.nhans_last_error()


@pytest.mark.parametrize("rate,L", [(48000, 17), (44100, 17), (22050, 0), (96000, 5)])
def test_a_simulated_hold_never_overflows(lib_built, rate, L):
    """The host's bookkeeping replayed for random cuttings: a push of a running stream keeps [E_new, N_new), which fits H,
    and every output it emits finds its input sample in the old half or in the push."""
    H = live.fullband_hold(rate)
    rng = np.random.default_rng(rate + L)
    for trial in range(6):
        N = E = base = 0
        most = 0
        for _ in range(400):
            cnt = int(rng.choice([1, 7, rate // 100, rate // 143, 2003, rate // 4]))
            En = live.emitted(N + cnt, False, rate, rate, L)
            assert base <= E <= En <= N + cnt          # outputs [E, En) read samples >= base, below N + cnt
            keep = min(En, N + cnt)
            assert N + cnt - keep <= H
            most = max(most, N + cnt - keep)
            N, E, base = N + cnt, En, keep
        assert L < 17 or most > H // 2             # (the bound is the longest look-ahead's)


def test_refusals_before_a_device(lib_built):
    lib = hip.load()
    assert lib.nhans_fullband_live_enable(None, None) == -1 and b"nhans_fullband_live_enable" in lib.nhans_last_error()
    assert lib.nhans_fullband_live_set_gain(None, 0, 1.0) == -1 and b"nhans_fullband_live_set_gain" in lib.nhans_last_error()
    off = hip.i64_array([0, 0])
    assert lib.nhans_fullband_mix(None, None, 0, off, None, None, off, 1, 48000, 1.0, 0.0, None, 1.0, 1.0, 0, None, off, None) == -1


@pytest.mark.parametrize("rate", [32000, 44100, 48000])
def test_the_complement_in_float64(rate):
    """u - R(R_in(u)) relative to a sine tone u, RMS over the middle half (away from the clip's edges): at most 3e-3 at 1
    and 6 kHz -- the pass-band ripple of the two Kaiser low-passes, about -53 dB --, at least 0.99 at 12 kHz."""
    for hz, lo, hi in ((1000.0, 0.0, 3e-3), (6000.0, 0.0, 3e-3), (12000.0, 0.99, 1.01)):
        u = F.tone(rate, hz)
        r = u - F.round_trip64(u, rate)
        a, b = len(u) // 4, 3 * len(u) // 4
        rel = F.rms(r[a:b]) / F.rms(u[a:b])
        print("%d Hz tone at %d Hz: |u - R(R_in(u))| / |u| = %.3e" % (hz, rate, rel))
        assert lo <= rel <= hi, (rate, hz, rel)


def test_restatements_agree():
    """The float32 restatement pieces against the float64 one on random data, R taken out (gain on the input alone):
    with den = mix = 0 the float64 restatement is g * x / in_denom."""
    rng = np.random.default_rng(5)
    x = rng.integers(-20000, 20000, 4800).astype(np.int16)
    z = np.zeros(1600, np.float32)
    y64 = F.restate64(x, z, z, 48000, 21000.000001, 0.3, 0.7)
    y32 = F.add_high32(np.zeros(4800, np.float32), x, 21000.000001, 0.7)
    assert len(y64) == len(y32) == 4800 and np.abs(y32 - y64).max() <= 2.0 ** -23
    assert np.array_equal(F.pcm(F.add_high32(np.zeros(4800, np.float32), x, 21000.000001, 1.0), np.int16, 21000.000001), x)


def test_cli_refuses_other_combinations(tmp_path):
    wav = str(tmp_path / "in.wav")          # (a path that is no directory: the parser's defaults are the process-wide flags)
    ok = ["--input", wav, "--highband", "1", "--output_rate", "input", "--convert_on", "gpu"]
    saved = {k: getattr(apply.FLAGS, k) for k in ("input", "highband", "output_rate", "convert_on", "convert")}
    try:
        assert apply._parse(ok, "nhans_denoiser").highband == 1.0
        for argv in (ok[:4], ok[:6], ok[:4] + ok[6:], ok + ["--no-convert"], ok[:3] + ["4.5"] + ok[4:], ok[:3] + ["-0.1"] + ok[4:],
                     ["--input", str(tmp_path)] + ok[2:]):
            with pytest.raises(SystemExit):
                apply._parse(argv, "nhans_denoiser")
        assert apply._parse(ok[:2], "nhans_denoiser").highband is None
    finally:
        for k, v in saved.items():
            setattr(apply.FLAGS, k, v)
