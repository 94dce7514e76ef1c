"""BSS Eval, the host side: the C ABI's surface and refusals, the float64 definition (nhans_amd.score.bss_reference) against
a dense least-squares formulation, its invariances, the condition that keeps the bar honest on every test clip, the bar's
sight of planted faults (tests/bss_checks.py), and the record helpers.  The device side: tests/test_gpu_bss.py."""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import nhans_amd  # noqa: F401
from nhans_amd import hip, score

import bss_checks as B


# ------------------------------------------------------------------------------ surface
def test_header_table_and_signature_agree(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    assert int(re.search(r"#define NHANS_BSS_FIELDS (\d+)", header).group(1)) == hip.BSS_FIELDS == 16
    assert len(score.BSS_FIELDS) == 13                                                      # the rest of a record is zero
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    names = re.findall(r"\b(nhans_[a-z_0-9]+)\s*\(", code)
    assert names.index("nhans_stoi") < names.index("nhans_bss_eval") < names.index("nhans_profile_json")
    assert len(hip.SIGNATURES["nhans_bss_eval"][1]) == 11
    kernels = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    assert "kBssFields = 16" in kernels and "kBssMaxL = %d" % score.BSS_MAX_FILTER in kernels
    assert "kBssCorrTile = %d" % B.CORR_TILE in kernels and "kBssProjTile = %d" % B.PROJ_TILE in kernels
    lib = hip.load()
    assert lib.nhans_abi_version() == 5 and re.search(r"#define NHANS_ABI_VERSION 5\b", header)
    assert hasattr(lib, "nhans_bss_eval")


def test_refusals_before_the_device_is_touched(lib_built):
    """Every argument check comes before the context is looked at: a NULL context is only reported for a call that has
    nothing else wrong."""
    lib = hip.load()
    B.check_refusals(lib, None)
    from nhans_amd import context
    import ctypes
    buf = ctypes.c_void_p(4096)
    assert context.bss_call(lib, None, buf, [0, 10], [buf], [[0, 10]], 1, 16, buf, None, None) < 0      # the context, last


# ------------------------------------------------------------------------------ the definition
def _dense(e, sources, L):
    """The same figures from the (n + L - 1) x J L matrix of the shifted sources and np.linalg.lstsq."""
    n = len(e)
    e64 = np.concatenate([np.asarray(e, np.float64), np.zeros(L - 1)])
    cols = [np.concatenate([np.zeros(b), np.asarray(s, np.float64), np.zeros(L - 1 - b)]) for s in sources for b in range(L)]
    S = np.stack(cols, axis=1)
    P = S @ np.linalg.lstsq(S, e64, rcond=None)[0]
    st = S[:, :L] @ np.linalg.lstsq(S[:, :L], e64, rcond=None)[0]
    return dict({"n": n, "J": len(sources), "L": L, "singular": 0}, **score.bss_figures(np.asarray(e, np.float64), P, st, L))


@pytest.mark.parametrize("L,J,n,a", [(1, 1, 50, 0.5), (4, 2, 200, 0.9), (16, 2, 700, 0.5), (16, 1, 40, 0.9), (33, 2, 1000, 0.99)])
def test_reference_against_dense_least_squares(L, J, n, a):
    e, src = B.clip(n, a, 500 + L, J)
    r = B.bss_ratios(_dense(e, src, L), e, src, L)
    print("bss reference against lstsq L %d J %d n %d: worst ratio to the bar %.3g" % (L, J, n, max(r.values())))
    assert max(r.values()) <= 1.0, r
    ref = score.bss_reference(e, src, L)
    assert all(math.isfinite(ref[k]) for k in score.BSS_ENERGIES) and ref["sdr_db"] < ref["sar_db"] + 1e-9


def test_every_shape_meets_the_condition_and_the_cap():
    """Condition 1 on every clip the device test holds to the bar, and no figure dropped but the named ones."""
    for shape in B.SHAPES:
        if shape[0] * shape[1] > 200 and shape[2] > 4000:
            continue                                         # (the largest: left to the device test, which computes it anyway)
        e, src = B.shape_clip(shape)
        ref, bar = B.bss_bar(e, src, shape[0])
        assert bar is not None and ref["singular"] == 0, shape
        r = B.bss_ratios(ref, e, src, shape[0], may_drop=B.may_drop(shape), ref=ref)
        assert max(r.values()) == 0.0
        for k in score.BSS_FIGURES:
            if k not in B.may_drop(shape) and math.isfinite(ref[k]):
                assert bar[k] < B.CAP, (shape, k, bar[k])


def test_one_source_and_edges():
    e, (s0, s1) = B.clip(900, 0.9, 601)
    one = score.bss_reference(e, [s0], 16)
    assert one["J"] == 1 and one["E_int"] == 0.0 and one["sir_db"] == math.inf and one["sar_db"] == one["sdr_db"]
    two = score.bss_reference(e, [s0, s1], 16)
    assert two["sar_db"] > one["sar_db"] and math.isfinite(two["sir_db"])               # the interferer explains part of the rest
    for rec in (score.bss_reference(e, [s0, np.zeros_like(s1)], 16), score.bss_reference(e[:0], [s0, s1], 16),
                score.bss_reference(e, [np.zeros_like(s0)], 4)):
        assert rec["singular"] == 1 and all(math.isnan(rec[k]) for k in score.BSS_ENERGIES + score.BSS_FIGURES)
    assert score.bss_reference(e[:0], [s0, s1], 16)["n"] == 0 and score.bss_reference(e, [s0[:700], s1], 16)["n"] == 700
    with pytest.raises(ValueError):
        score.bss_reference(e, [s0, s1, s1], 16)
    with pytest.raises(ValueError):
        score.bss_reference(e, [s0], 513)


def test_invariances():
    L = 16
    e, (s0, s1) = B.clip(1500, 0.9, 602)
    ref, bar = B.bss_bar(e, [s0, s1], L)
    # a source scaled by a power of two
    for k0, k1 in ((8.0, 1.0), (1.0, 0.125), (0.5, 4.0)):
        got = score.bss_reference(e, [s0 * np.float32(k0), s1 * np.float32(k1)], L)
        r = {k: B.ratio(got[k], ref[k], bar[k]) for k in score.BSS_FIGURES}
        r.update({k: B.ratio(got[k] / ref["E_e"], ref[k] / ref["E_e"], bar[k]) for k in score.BSS_ENERGIES})
        assert max(r.values()) <= 1.0, (k0, k1, r)
    # the estimate's target part filtered by a short FIR: the artifact energy stays.  Everything on a grid of 2^-16 so that
    # the filtered estimate is exact in float32, and the target's last taps - 1 samples zero so that it ends with the clip.
    rng = np.random.default_rng(603)
    q = lambda x, bits: (np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits)
    t0, t1, w = q(B.ar1(1500, 0.9, rng) * 4, 12), q(B.ar1(1500, 0.9, rng) * 4, 12), q(0.05 * rng.standard_normal(1500), 16)
    t0[-2:] = 0.0
    h = np.array([1.0, 0.5, 0.25])
    ea = (t0 + 0.25 * t1 + w).astype(np.float32)
    eb = (np.convolve(h, t0)[:1500] + 0.25 * t1 + w).astype(np.float32)
    assert np.array_equal(eb.astype(np.float64), np.convolve(h, t0)[:1500] + 0.25 * t1 + w)
    src = [t0.astype(np.float32), t1.astype(np.float32)]
    ra, ba = B.bss_bar(ea, src, L)
    rb, bb = B.bss_bar(eb, src, L)
    assert abs(ra["E_art"] - rb["E_art"]) <= ba["E_art"] * ra["E_e"] + bb["E_art"] * rb["E_e"]
    assert abs(ra["E_tgt"] - rb["E_tgt"]) > 1e6 * (ba["E_tgt"] * ra["E_e"] + bb["E_tgt"] * rb["E_e"])   # (the target part did change)


# ------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", [B.fault_lag_off_in_r01, B.fault_unpadded_estimate, B.fault_c0_from_c, B.fault_projection_cut])
def test_the_bar_sees_a_planted_fault(fault):
    L = 16
    e, src = B.clip(1200, 0.9, 604)
    ref, bar = B.bss_bar(e, src, L)
    got = fault(e, src, L)
    r = {k: B.ratio(got[k] / ref["E_e"], ref[k] / ref["E_e"], bar[k]) for k in score.BSS_ENERGIES}
    r.update({k: B.ratio(got[k], ref[k], bar[k]) for k in score.BSS_FIGURES})
    print("bss fault %s: worst ratio to the bar %.3g" % (fault.__name__, max(r.values())))
    assert max(r.values()) > 1e3, r


# ------------------------------------------------------------------------------ records
def test_merge_and_improvement_keys():
    vals = np.arange(16, dtype=np.float64)
    rec = score.bss_record(vals)
    assert tuple(rec) == score.BSS_FIELDS and isinstance(rec["n"], int) and isinstance(rec["singular"], int) and rec["sdr_db"] == 9.0
    plain = {"n": 5, "si_sdr_db": 1.0, "snr_db": 2.0, "segsnr_db": 3.0, "loss": 2.0}
    merged = score.merge_bss(plain, rec)
    assert set(merged) == set(plain) | {"bss_n"} | (set(score.BSS_FIELDS) - {"n"}) and merged["n"] == 5 and merged["bss_n"] == 0
    after = score.merge_bss(dict(plain, si_sdr_db=4.0, loss=1.0), score.bss_record(vals + 1.5))
    imp = score.improvement(merged, after)
    assert set(imp) == {"si_sdr_i", "snr_i", "segsnr_i", "loss_ratio", "sdr_i", "sir_i", "sar_i"}
    assert imp["sdr_i"] == imp["sir_i"] == imp["sar_i"] == 1.5 and imp["si_sdr_i"] == 3.0
    # unchanged where one of the records has no such figures
    assert set(score.improvement(plain, after)) == set(score.improvement(merged, plain)) == {"si_sdr_i", "snr_i", "segsnr_i", "loss_ratio"}
    assert score.improvement(plain, dict(plain, loss=1.0)) == {"si_sdr_i": 0.0, "snr_i": 0.0, "segsnr_i": 0.0, "loss_ratio": 0.5}
