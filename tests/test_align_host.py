"""Delay estimation without a device: the float64 definition nhans_amd.score.align_reference on known answers and against
exact rational arithmetic, the bars of tests/align_checks.py against the planted faults (each factor is printed: pytest
-s), the kernel's constants, the header's prototypes and the command line's argument errors."""
import ctypes
import fractions
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, score

import align_checks as A


def test_known_answers_and_the_tie_rule():
    for k, (_, _, n, D, delay) in enumerate(A.TIE_CLIPS):
        e, t = A.tie_clip(k)
        r = score.align_reference(e, t, D, corr=True)
        assert r["delay"] == delay and r["n_common"] == n - abs(delay) and (r["ne"], r["nt"], r["D"]) == (n, n, D)
        assert A.delay_is_decided(e, t, r, A.corr_bars(e, t, D)) == "exact"
    e, t = A.tie_clip(0)
    r = score.align_reference(e, t, 6, corr=True)
    assert r["corr"][6 + 3] == 1.0 and r["corr"][6 - 3] == 1.0 and r["c_peak"] == 1.0 and r["rho"] == 1.0 / math.sqrt(2.0)
    r = score.align_reference(*A.tie_clip(2), 6)
    assert r["delay"] == 0 and math.isnan(r["rho"]) and r["c_peak"] == 0.0
    # the sign convention: a late estimate has a positive delay, and the cut pair lines up
    e, t = A.delayed_pair(300, 280, 17, 1, noise=0.0)
    assert score.align_reference(e, t, 40)["delay"] == 17
    ec, tc = score.align_cut(e, t, 17)
    assert len(ec) == len(tc) == 280 and np.array_equal(ec, tc)
    e, t = A.delayed_pair(300, 280, -9, 2, noise=0.0)
    assert score.align_reference(e, t, 40)["delay"] == -9
    ec, tc = score.align_cut(e, t, -9)
    assert len(ec) == len(tc) == 271 and np.array_equal(ec, tc)
    # an empty range is +0.0, and lags past either clip are empty
    r = score.align_reference(np.ones(2, np.float32), np.ones(3, np.float32), 5, corr=True)
    assert r["corr"].tolist() == [0, 0, 0, 1, 2, 2, 1, 0, 0, 0, 0] and not np.signbit(r["corr"]).any() and r["delay"] == 0
    assert score.align_common(10, 12, -3) == 9 and score.align_common(5, 5, 9) == 0 and score.align_common(0, 7, 0) == 0
    with pytest.raises(ValueError):
        score.align_cut(e, t, 301)
    with pytest.raises(ValueError):
        score.align_reference(e, t, 16001)
    rec = score.align_record([7.0, 9.0, 3.0, -2.0, 0.5, 0.25, 7.0, 0.0])
    assert rec == {"ne": 7, "nt": 9, "D": 3, "delay": -2, "c_peak": 0.5, "rho": 0.25, "n_common": 7} and tuple(rec) == score.ALIGN_FIELDS
    assert hip.ALIGN_FIELDS == 8 and score.ALIGN_MAX_LAG == hip.ALIGN_MAX_LAG == 16000


def test_reference_against_exact_rational_arithmetic():
    e, t = A.delayed_pair(37, 45, 5, 3)
    D = 50
    r = score.align_reference(e, t, D, corr=True)
    ef, tf = [fractions.Fraction(float(x)) for x in e], [fractions.Fraction(float(x)) for x in t]
    for d in range(-D, D + 1):
        acc = fractions.Fraction(0)
        for u in range(len(tf)):
            if 0 <= u + d < len(ef):
                acc += ef[u + d] * tf[u]
        assert r["corr"][d + D] == float(acc), d
    assert r["delay"] == 5 and r["c_peak"] == r["corr"].max()
    See, Stt = float(sum(x * x for x in ef)), float(sum(x * x for x in tf))
    assert r["rho"] == r["c_peak"] / math.sqrt(See * Stt)


def test_the_issues_delayed_copy_and_the_device_order_on_the_host():
    """A copy delayed by 211 samples plus noise at half its level, n = 5000, D = 600: the winner's lead in bars, and the
    device's order of adding (align_checks.device_order_corr, bit for bit what align.hip computes) against the bar."""
    e, t = A.delayed_pair(5000, 5000, 211, 4)
    r = score.align_reference(e, t, 600, corr=True)
    bars = A.corr_bars(e, t, 600)
    lead = A.delay_is_decided(e, t, r, bars)
    dev = A.device_order_corr(e, t, 600)
    got = A.align_ratios(dict(r, c_peak=float(dev[211 + 600])), dev, e, t, r, bars)
    print("align host: delay %d, lead %.3g bars, device order at %.3g of the bar" % (r["delay"], lead, got["corr"]))
    assert r["delay"] == 211 and lead > 1e9 and got["corr"] <= 0.5


def test_every_shape_is_decided_on_the_reference_alone():
    leads = {}
    for i, s in enumerate(A.SHAPES):
        e, t, ref, bars, how = A.shape_reference(i)
        assert (len(e), len(t)) == s[:2] and A.is_exact(e, t) == s[4]
        if abs(s[3]) <= s[2] and min(s[:2]) > 2:
            assert ref["delay"] == s[3], (s, ref["delay"])
        leads[str(s[:4])] = how
    print("align shapes: the winner's lead in bars", leads)
    assert any(s[2] > max(s[:2]) for s in A.SHAPES) and any(abs(s[3]) > s[2] for s in A.SHAPES)


def test_the_bar_sees_the_planted_faults():
    e, t = A.delayed_pair(A.TS + 300, A.TS + 310, 40, 5)
    D = 64
    ref = score.align_reference(e, t, D, corr=True)
    bars = A.corr_bars(e, t, D)
    assert A.align_ratios(ref, ref["corr"], e, t, ref, bars) == {"corr": 0.0, "rho": 0.0}
    factors = {}
    for fault in (A.fault_sample_dropped_at_tile_edge, A.fault_lag_table_off_by_one, A.fault_swapped):
        rec, c = fault(e, t, D)
        diff = np.abs(c - ref["corr"])
        factors[fault.__name__] = float((diff / bars).max())
        if rec["delay"] == ref["delay"]:
            with_bar = A.align_ratios(rec, c, e, t, ref, bars)
            assert with_bar["corr"] == factors[fault.__name__]
        else:
            with pytest.raises(AssertionError):
                A.align_ratios(rec, c, e, t, ref, bars)
    # the tie rule is held by equality on the exact clips: reversed, the first of them answers -3 and the third -6
    for k, wrong in ((0, -3), (2, -6)):
        et = A.tie_clip(k)
        D = A.TIE_CLIPS[k][3]
        ref_k = score.align_reference(*et, D, corr=True)
        rec, c = A.fault_tie_rule_reversed(*et, D)
        assert rec["delay"] == wrong != ref_k["delay"]
        with pytest.raises(AssertionError):
            A.align_ratios(rec, c, *et, ref_k, A.corr_bars(*et, D))
    print("align planted faults: worst |c - c_ref| over its bar", factors)
    assert min(factors.values()) > 1e6, factors


def test_constants_match_the_kernel():
    k = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    m = re.search(r"kAlignFields = (\d+), kAlignMaxLag = (\d+), kAlignTile = (\d+), kAlignLagBlock = (\d+)", k)
    assert m and tuple(int(v) for v in m.groups()) == (hip.ALIGN_FIELDS, hip.ALIGN_MAX_LAG, A.TS, A.LB)
    text = open(os.path.join(ROOT, "n-hans_amd", "csrc", "align.hip")).read()
    assert "kAlignLagBlock == 256 * kAlignRL" in text and re.search(r"kAlignRL = (\d+)", text).group(1) == str(A.LB // 256)
    assert "kAlignTile = 2,048" in text                     # (the stated order names the tile)
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    assert "#define NHANS_ALIGN_FIELDS %d" % hip.ALIGN_FIELDS in header and "#define NHANS_ALIGN_MAX_LAG %d" % hip.ALIGN_MAX_LAG in header
    assert len(score.ALIGN_FIELDS) == 7


def test_prototypes_and_signature_table_agree():
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    restypes = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name, ret, nargs in (("nhans_align", "int", 10), ("nhans_align_common", "int64_t", 3), ("nhans_align_cut", "int", 11)):
        m = re.search(r"([A-Za-z_0-9]+)\s+%s\s*\(([^()]*)\)\s*;" % name, code)
        assert m and m.group(1) == ret and m.group(2).count(",") + 1 == nargs, name
        restype, argtypes = hip.SIGNATURES[name]
        assert restype is restypes[ret] and len(argtypes) == nargs, name


def test_library_refuses_without_a_device(lib_built):
    A.check_refusals(hip.load(), None)


def test_cli_argument_errors(tmp_path):
    wav, tgt = str(tmp_path / "in.wav"), str(tmp_path / "t.wav")
    open(tgt, "wb").close()
    keys = ("input", "score_against", "align_ms")
    saved = {k: getattr(apply.FLAGS, k) for k in keys}
    try:
        for prog in ("nhans_denoiser", "nhans_separator"):
            a = apply._parse(["--input", wav, "--score_against", tgt, "--align_ms", "10"], prog)
            assert a.align_ms == 10.0 and int(round(16 * a.align_ms)) == 160
            assert apply._parse(["--input", wav, "--score_against", tgt], prog).align_ms is None
            for argv in (["--input", wav, "--align_ms", "10"], ["--input", wav, "--score_against", tgt, "--align_ms", "0"],
                         ["--input", wav, "--score_against", tgt, "--align_ms", "-3"],
                         ["--input", wav, "--score_against", tgt, "--align_ms", "1000.5"]):
                with pytest.raises(SystemExit):
                    apply._parse(argv, prog)
            assert apply._parse(["--input", wav, "--score_against", tgt, "--align_ms", "1000"], prog).align_ms == 1000.0
    finally:
        for k, v in saved.items():
            setattr(apply.FLAGS, k, v)
