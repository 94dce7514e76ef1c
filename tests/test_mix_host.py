"""Mixing at a chosen SNR, the host side: the C ABI's surface and refusals, the host's SNR factor against Python's pow, the
restatement of the rule with explicit dtypes (tests/mix_checks.py) against nhans_amd.mixing bit for bit, the identity
behind `unit`, the SNR a mixture really has, and the comparison's sight of planted faults.  The device side:
tests/test_gpu_mix.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import nhans_amd  # noqa: F401
from nhans_amd import hip, mixing

import mix_checks as M


@pytest.fixture(scope="module")
def cases():
    """(case, restatement) pairs, computed once."""
    return [(c, M.reference(c[1], c[2], c[3], c[4], c[5])) for c in M.host_cases()]


# ------------------------------------------------------------------------------ surface
def test_surface(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    assert int(re.search(r"#define NHANS_MIX_FIELDS (\d+)", header).group(1)) == hip.MIX_FIELDS == 8
    assert len(mixing.RECORD_FIELDS) == 7 and mixing.RECORD_FIELDS == M.FIELDS          # the eighth double is zero
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, nargs in (("nhans_mix_snr_factor", 2), ("nhans_mix", 20)):
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, code).group(1)
        assert params.count(",") + 1 == nargs == len(hip.SIGNATURES[name][1]), name
        assert name in hip.EXPORTS
    names = list(hip.SIGNATURES)
    assert names.index("nhans_score_rows") < names.index("nhans_mix_snr_factor") < names.index("nhans_mix") < names.index("nhans_profile_json")
    kernels = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    assert "kMixTile = %d" % hip.MIX_TILE in kernels and "kMixFields = 8" in kernels
    lib = hip.load()
    assert lib.nhans_abi_version() == 5 == hip.ABI_VERSION
    assert hasattr(lib, "nhans_mix") and hasattr(lib, "nhans_mix_snr_factor")


def snr_factor(lib, snr):
    f = ctypes.c_double(0.0)
    assert lib.nhans_mix_snr_factor(float(snr), ctypes.byref(f)) == 0
    return f.value


def test_snr_factor_is_pythons_pow(lib_built):
    lib = hip.load()
    snrs = [k * 0.5 for k in range(-60, 61)] + mixing.SNRS_DENOISER + mixing.SNRS_SEPARATOR
    assert len(snrs) == 121 + 5 + 7
    for snr in snrs:
        want = pow(10, -snr / 10.0)
        assert snr_factor(lib, snr).hex() == want.hex() == M.snr_factor(snr).hex(), snr
    assert lib.nhans_mix_snr_factor(0.0, None) == -1 and "null output" in lib.nhans_last_error().decode()


# ------------------------------------------------------------------------------ the restatement
def test_restatement_is_the_host_rule_bit_for_bit(cases):
    for (name, s, a, b, sk, sd, _), ref in cases:
        mixture, target, gk, gd, keep, drop = mixing.domixing(s, a, b, sk, sd)
        for got, key in ((mixture, "mixture"), (target, "target"), (keep, "keep"), (drop, "drop")):
            assert got.dtype == np.float32 and M.same_bits(got, ref[key]), (name, key)
        assert float(gk).hex() == ref["g_keep"].hex() and float(gd).hex() == ref["g_drop"].hex(), name
        # the powers the record holds are the ones the host rule divides
        n = len(s)
        assert float(mixing._mean_power(s)).hex() == ref["P_s"].hex(), name
        assert float(mixing._mean_power(mixing._fit_length(a, n))).hex() == ref["P_keep"].hex(), name
        assert float(mixing._mean_power(mixing._fit_length(b, n))).hex() == ref["P_drop"].hex(), name
        # the separator's two-way mix
        two = M.reference(s, None, b, None, sd)
        mixture2, g2 = mixing.domixing_separator(s, b, sd)
        assert M.same_bits(mixture2, two["mixture"]) and float(g2).hex() == two["g_drop"].hex(), name
        assert (two["P_keep"], two["g_keep"]) == (0.0, 1.0) and not two["keep"].any()
        assert M.same_bits(two["target"], s / np.float32(two["unit"])), name


def test_unit_is_the_peak_of_the_normalised_mixture(cases):
    """unit = float32(float32(pk / p) + 1e-6f) needs no second pass over the data: correctly rounded division is
    monotone, so max |raw / p| = max |raw| / p."""
    for (name, *_), ref in cases:
        peak = mixing._peak(ref["mixture"])
        assert isinstance(peak, np.float32) and float(peak) == ref["unit"], name
    z = M.reference(np.zeros(5, np.float32), np.zeros(2, np.float32), np.zeros(9, np.float32), 0, 0)
    assert z["pk"] == 0.0 and z["unit"] == float(np.float32(1e-6)) and not z["mixture"].any() and not z["target"].any()
    assert (z["g_keep"], z["g_drop"]) == (1.0, 1.0)


def test_achieved_snr(cases):
    """10 log10(sum s^2 / sum (g32 A)^2) in float64 against the SNR asked for: the float32 rounding of the gain alone is
    5.2e-7 dB (20 / ln 10 x 2^-24); 1e-5 dB leaves room for the products' roundings."""
    worst, seen = 0.0, 0
    for (name, s, a, b, sk, sd, plain), ref in cases:
        if not plain:
            continue
        for g, x, snr in ((ref["g_keep"], a, sk), (ref["g_drop"], b, sd)):
            err = abs(M.achieved_snr_db(s, g, M.fit(x, len(s))) - snr)
            worst, seen = max(worst, err), seen + 1
            assert err <= 1e-5, (name, snr, err)
    print("achieved SNR: worst |error| %.3g dB over %d gains" % (worst, seen))
    assert seen >= 40


# ------------------------------------------------------------------------------ planted faults
def test_the_comparison_sees_planted_faults():
    n = 2 * hip.MIX_TILE + 1
    s, a, b = M.signal(n, 1), M.signal(700, 2, 0.1), M.signal(n + 5, 3, 0.7)
    ref = M.reference(s, a, b, 3, -3)
    again = M.reference(s, a, b, 3, -3)
    assert all(M.same_bits(ref[k], again[k]) for k in M.OUTPUTS) and all(ref[k] == again[k] for k in M.FIELDS)

    def differing(got, key):
        return int(np.count_nonzero(M.bits(got[key]) != M.bits(ref[key])))

    # a pairwise sum in place of the chain: the float32 gains may coincide, the record's float64 powers do not
    # (on 32,400 terms the chain's rounding errors walk away from the exact sum and a pairwise sum's stay within a few
    # 2^-53 of it: the two come out a few ulps apart, and the comparison is exact, so one ulp on each power is seen)
    ls, la, lb = M.signal(32400, 11), M.signal(5000, 12, 0.1), M.signal(40000, 13, 0.7)
    chain, pair = M.reference(ls, la, lb, 3, -3), M.reference(ls, la, lb, 3, -3, fault="pairwise_power")
    ulps = {k: M.ulps64(pair[k], chain[k]) for k in ("P_s", "P_keep", "P_drop")}
    print("pairwise sum: powers off by", ulps, "ulps")
    assert min(ulps.values()) >= 1
    print("pairwise sum: mixture samples that differ:", int(np.count_nonzero(M.bits(pair["mixture"]) != M.bits(chain["mixture"]))))
    # a gain applied in double: one rounding instead of the float32 gain's two (the comparison is exact, so one sample
    # would do; hundreds of each output move)
    got = M.reference(s, a, b, 3, -3, fault="gain_in_double")
    cnt = {k: differing(got, k) for k in M.OUTPUTS}
    print("gain in double: samples that differ", cnt, "of", n)
    assert min(cnt.values()) > 0
    # the target divided by p instead of unit
    got = M.reference(s, a, b, 3, -3, fault="target_by_p")
    cnt = {k: differing(got, k) for k in ("target", "keep", "drop")}
    rel = float(np.max(np.abs(got["target"] - ref["target"])) / np.max(np.abs(ref["target"])))
    print("target by p: samples that differ", cnt, "relative error %.3g" % rel)
    assert min(cnt.values()) > n // 2 and rel > 0.05 and differing(got, "mixture") == 0
    # a fit that restarts the noise at every tile: everything from the second tile on
    got = M.reference(s, a, b, 3, -3, fault="fit_restarts_per_tile", tile=hip.MIX_TILE)
    cnt = {k: differing(got, k) for k in M.OUTPUTS}
    print("fit restarts per tile: samples that differ", cnt)
    assert min(cnt.values()) > n // 4 and got["P_keep"] != ref["P_keep"] and got["P_drop"] != ref["P_drop"]


# ------------------------------------------------------------------------------ refusals
def test_refusals_before_the_device_is_touched(lib_built):
    """Every argument check comes before the context is looked at: a NULL context is only reported for a call that has
    nothing else wrong."""
    lib = hip.load()
    buf = ctypes.c_void_p(4096)            # a pointer that is never followed
    off = hip.i64_array

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def dbls(*v):
        return (ctypes.c_double * len(v))(*v)

    def err():
        return lib.nhans_last_error().decode()

    def call(speech=buf, soff=off([0, 10, 10]), nspeech=2, noise=buf, noff=off([0, 4, 4, 30]), nnoise=3, si=ints(0, 0), ki=ints(0, -1),
             di=ints(2, 2), sk=dbls(0, 0), sd=dbls(3, 3), njobs=2, mixture=buf, target=None, keep=None, drop=None,
             ooff=off([0, 10, 20]), rec=None):
        return lib.nhans_mix(None, speech, soff, nspeech, noise, noff, nnoise, si, ki, di, sk, sd, njobs, mixture, target, keep, drop,
                             ooff, rec, None)

    assert call(njobs=-1) == -1 and "negative job count" in err()
    assert call(nnoise=-1) == -1 and "negative clip count" in err()
    for null in ("speech", "soff", "noise", "noff", "si", "di", "sd", "mixture", "ooff"):
        assert call(**{null: None}) == -1 and "null" in err(), null
    assert call(sk=None) == -1 and "job 0" in err() and "no keep SNRs" in err()
    assert call(si=ints(0, 2)) == -1 and "job 1" in err() and "speech index 2" in err()
    assert call(si=ints(-1, 0)) == -1 and "job 0" in err() and "speech index -1" in err()
    assert call(ki=ints(0, 3)) == -1 and "job 1" in err() and "keep index 3" in err()
    assert call(ki=ints(-2, 0)) == -1 and "job 0" in err() and "keep index -2" in err()
    assert call(di=ints(2, 3)) == -1 and "job 1" in err() and "drop index 3" in err()
    assert call(si=ints(0, 1)) == -1 and "job 1" in err() and "speech clip 1 has 0 samples" in err()
    assert call(ki=ints(1, -1)) == -1 and "job 0" in err() and "keep noise clip 1 has 0 samples" in err()
    assert call(di=ints(2, 1)) == -1 and "job 1" in err() and "drop noise clip 1 has 0 samples" in err()
    assert call(ooff=off([0, 10, 19])) == -1 and "job 1" in err() and "room for 9 of 10" in err()
    # nothing wrong but the context (a NULL keep index array: every job two-way; no job: nothing is needed)
    assert call() == -1 and "null context" in err()
    assert call(ki=None, sk=None) == -1 and "null context" in err()
    assert lib.nhans_mix(None, None, None, 0, None, None, 0, None, None, None, None, None, 0, None, None, None, None, None, None,
                         None) == -1 and "null context" in err()
