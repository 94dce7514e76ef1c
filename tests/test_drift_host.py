"""Drift-aware alignment without a device: the float64 definition (nhans_amd.score.drift_reference, drift_fit,
drift_warp_reference) on analytic clips whose line is known, the host-only calls of the library (table, segments, range,
fit) against their restatements, the bars of tests/drift_checks.py against the planted faults (each factor is printed:
pytest -s), the kernel's constants, the header's prototypes, the refusals and the command line's argument errors."""
import ctypes
import ctypes.util
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import nhans_amd  # noqa: F401
from nhans_amd import apply, context, hip, score

import drift_checks as C


def lib_range(ne, nt, a, b):
    lo, hi = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert hip.load().nhans_drift_range(ne, nt, a, b, ctypes.byref(lo), ctypes.byref(hi)) == 0, hip.load().nhans_last_error()
    return lo.value, hi.value


def test_fused_multiply_add_of_the_definition_is_the_real_one():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype, libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    rng = np.random.default_rng(11)
    n = 20000
    a, b, c = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n)) for _ in range(3))
    c[:8000] = -(a[:8000] * b[:8000]) * (1 + rng.integers(-3, 4, 8000) * 2.0 ** -52)       # cancellation to the last bits
    a[8000:10000] = a[8000:10000].astype(np.float32)
    c[10000:11000] = 0.0
    got = score._fma(a, b, c)
    ref = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert C.same_bits(got, ref)
    assert float(score._fma(3.0, 0.0, 0.0)) == 0.0 and not np.signbit(score._fma(-3.0, 0.0, 0.0))


def test_table_against_the_numpy_design(lib_built):
    G, D = score.drift_table()
    LG, LD = score.drift_library_table()
    assert LG.shape == (C.Q + 1, 2 * C.T) and LD.shape == (C.Q, 2 * C.T)
    worst = max(float(np.abs(G - LG).max()), float(np.abs(D - LD).max()))
    print("drift table: worst |library - numpy design| %.3e (bar 1e-15)" % worst)
    assert worst <= 1e-15
    assert LG[0].tolist() == [0.0] * (C.T - 1) + [1.0] + [0.0] * C.T and not np.signbit(LG[0]).any()
    assert C.same_bits(LD, LG[1:] - LG[:-1])
    assert abs(LG[C.Q, C.T] - 1.0) <= 1e-15 and np.abs(np.delete(LG[C.Q], C.T)).max() <= 1e-15        # row Q: the impulse one tap on
    # the interpolator itself: flat to 2e-5 up to 6.3 kHz at 16 kHz for every phase, and falling from there on
    w = 2 * np.pi * np.array([100.0, 1000.0, 3000.0, 5000.0, 6300.0]) / C.RATE
    k = np.arange(-C.T + 1, C.T + 1)
    for q in range(1, C.Q, 37):
        Hq = np.exp(-1j * np.outer(w, k - q / C.Q)) @ LG[q]
        assert np.abs(Hq - 1.0).max() <= 2e-5, (q, np.abs(Hq - 1.0).max())
    Hs = np.exp(-1j * 2 * np.pi * 7600.0 / C.RATE * (k - 0.5)) @ LG[C.Q // 2]
    assert abs(Hs) < 0.7
    assert score.drift_segments(C.B - 1) == 0 and score.drift_segments(C.B) == 1 and score.drift_segments(C.B + 2 * C.H) == 3
    for nt in (0, 1, C.B - 1, C.B, C.B + C.H - 1, C.B + C.H, 160000):
        assert hip.load().nhans_drift_segments(nt) == score.drift_segments(nt)


def test_range_at_exact_edges_and_the_position_with_one_rounding_fewer(lib_built):
    cases = [(100, 100, 0.0, 0.0), (100, 120, -3.0, 0.0), (100, 120, 3.0, 0.0), (0, 10, 0.0, 0.0), (10, 0, 0.0, 0.0), (1, 10, -3.0, 0.0),
             (1, 10, 0.5, 0.0), (32, 50, -10.0, 0.0), (100, 100, 200.0, 0.0), (100, 100, -200.0, 0.0),
             (5000, 5000, -2.0, 2.0 ** -10), (5000, 6000, 4.0, -2.0 ** -10),
             (4097, 5000, -1.0, 1.0 / 4096),        # p(4096) = 4096 = ne - 1 exactly
             (4097, 5000, 1.0, -1.0 / 4096),        # p(4096) = 4096 exactly, from above
             (3000, 3000, -2048.5, 2.0 ** -12),     # p(2048) = 0 exactly
             (2000, 1200, -23.0023, 1e-4)]          # p(23) = 0 exactly, after a rounding
    for ne, nt, a, b in cases:
        want = C.brute_range(ne, nt, a, b)
        assert lib_range(ne, nt, a, b) == want == score.drift_range(ne, nt, a, b), (ne, nt, a, b, want)
    assert float(score.drift_pos(-1.0, 1.0 / 4096, 4096.0)) == 4096.0 and lib_range(4097, 5000, -1.0, 1.0 / 4096) == (1, 4097)
    assert float(score.drift_pos(-2048.5, 2.0 ** -12, 2048.0)) == 0.0 and lib_range(3000, 3000, -2048.5, 2.0 ** -12)[0] == 2048
    # the planted fault: p as a + (1 + b) u.  It differs from the device's expression in the last bits of many positions,
    # and at an edge that is exactly 0 it moves the range -- the bar there is equality.
    a, b = -23.0023, 1e-4
    assert float(score.drift_pos(a, b, 23.0)) == 0.0 and float(C.fault_pos(a, b, 23.0)) < 0.0
    assert lib_range(2000, 1200, a, b) == C.brute_range(2000, 1200, a, b) == (23, 1200)
    assert C.brute_range(2000, 1200, a, b, pos=C.fault_pos) == (24, 1200)
    u = np.arange(40000.0)
    differs = int(np.count_nonzero(score.drift_pos(37.3, 50e-6, u) != C.fault_pos(37.3, 50e-6, u)))
    print("drift range: positions of 40000 whose bits differ under the planted expression:", differs)
    assert differs > 1000
    for bad in ((0, 0, math.nan, 0.0), (0, 0, 0.0, 0.002), (0, 0, 3e9, 0.0)):
        with pytest.raises(ValueError):
            score.drift_range(*bad)


def _rows(recs):
    return [[float(r[k]) for k in score.DRIFT_FIELDS] for r in recs]


def test_fit_is_the_restatement_bit_for_bit(lib_built):
    """nhans_drift_fit against score.drift_fit, bit for bit: host_drift.hip is compiled with contraction off (the pragma at its
    head), so the restatement's one-rounding-per-operation holds exactly and no bar applies."""
    text = open(os.path.join(ROOT, "n-hans_amd", "csrc", "host_drift.hip")).read()
    assert "#pragma clang fp contract(off)" in text.split("namespace {")[0]
    rng = np.random.default_rng(3)
    sets = [_rows([r[0] for r in C.reference_line(i)[1]]) for i in (0, 1)]
    for n in (0, 1, 2, 3, 4, 9, 40):
        u = np.arange(n) * 2048.0 + rng.uniform(1500, 2500, n)
        tau = 12.25 + 3e-4 * u + 0.01 * rng.standard_normal(n)
        rows = [[u[j], tau[j], rng.uniform(0.2, 1.0), rng.uniform(0.1, 9.0), 1.0, round(tau[j]), float(rng.integers(0, 8) == 0), 12.0] for j in range(n)]
        sets.append(rows)
    out = [dict(zip(score.DRIFT_FIELDS, r)) for r in sets[-1]]
    for j in (5, 17):
        out[j].update(flags=0.0, rho=0.9)
    out[5]["tau"] += 40.0                                   # an outlier the trimming pass drops
    out[17]["tau"] -= 3.0
    sets.append(_rows(out))
    sets.append([[100.0, 1.0, 0.9, 1.0, 1.0, 1.0, 0.0, 1.0]] * 5)                              # degenerate abscissae
    sets.append([[2048.0 * j, 3.0 * j, 0.9, 1.0, 1.0, 1.0, 0.0, 1.0] for j in range(6)])       # a slope beyond 2^-10
    sets.append([[2048.0 * j, 0.5, 0.9, 0.0, 1.0, 1.0, 0.0, 1.0] for j in range(6)])           # no weight at all
    sets.append([[math.nan, 0.5, math.nan, 0.0, 0.0, 1.0, 2.0, 1.0]] * 4)                      # silent segments
    seen = set()
    for rows in sets:
        for rho_min, trim in ((0.3, 1.0), (0.5, 0.02), (-1.0, 0.0)):
            got, ref = hip.drift_fit(rows, rho_min, trim), score.drift_fit(rows, rho_min, trim)
            assert tuple(got) == score.DRIFT_FIT_FIELDS == tuple(ref)
            for k in got:
                assert float(got[k]).hex() == float(ref[k]).hex() or (math.isnan(got[k]) and math.isnan(ref[k])), (k, got, ref)
            seen.add((got["fit_ok"], got["n_used"] < got["n_valid"], math.isnan(got["a"])))
    assert {(1, False, False), (1, True, False), (0, False, True), (0, False, False)} <= seen, seen
    f = score.drift_fit(sets[-4])
    assert f["fit_ok"] == 0 and math.isnan(f["a"]) and f["n_used"] == 5
    f = score.drift_fit(sets[-3])
    assert f["fit_ok"] == 0 and abs(f["b"] - 3.0 / 2048) < 1e-12
    f = score.drift_fit(sets[-5])
    assert f["fit_ok"] == 1 and f["n_used"] <= f["n_valid"] - 2 and abs(f["b"] - 3e-4) < 1e-5


def test_known_answers_of_the_reference():
    """The reference alone on clips whose line is known analytically.  What is asked of it: every listed clip fits
    (fit_ok, at least 80 % of its segments used); the fitted line stays within 0.05 sample of the true one at both ends
    of the clip; and the warped pair's SI-SDR is within 0.5 dB of what a timing error of 0.01 sample rms leaves below
    the clip's own noise -- a delay error d leaves a residual of (2 pi f d)^2 of the power at frequency f, 7.7e-5 at the
    clips' rms frequency of about 2.2 kHz -- and more than 3 dB above the best whole-sample alignment."""
    worst = {}
    for i, (n, a, b, snr, seed, max_lag, track_lag) in enumerate(C.E2E_CLIPS):
        e, t = C.e2e_clip(i)
        fit, refs, R, centre = C.reference_line(i)
        assert fit["fit_ok"] == 1 and fit["n_used"] >= 0.8 * len(refs) and len(refs) == score.drift_segments(n), (i, fit)
        assert all(r[1]["decided"] > 1.0 for r in refs if r[0]["flags"] == 0), i
        ends = max(abs(fit["a"] - a), abs((fit["a"] + fit["b"] * n) - (a + b * n)))
        y, lo, hi = score.drift_warp_reference(e, n, fit["a"], fit["b"])
        warped = C.si_sdr_db(y, t[lo:hi])
        ce, ct = score.align_cut(e, t, fit["d0"])
        whole = C.si_sdr_db(ce, ct)
        floor = -10.0 * math.log10(10.0 ** (-snr / 10.0) + 7.7e-5) - 0.5
        print("drift reference clip %d: a %.4f (true %.4f), b %.3f ppm (true %.1f), line off by %.4f at an end, used %d / %d, "
              "SI-SDR whole-sample %.2f dB, warped %.2f dB (asked: %.2f)" % (i, fit["a"], a, 1e6 * fit["b"], 1e6 * b, ends,
                                                                               fit["n_used"], len(refs), whole, warped, floor))
        worst[i] = ends / 0.05
        assert ends <= 0.05 and warped >= floor and warped > whole + 3.0, (i, ends, warped, floor, whole)
    print("drift reference: worst ratio of the line's end error to 0.05 sample", worst)
    # the sign convention: a late estimate has a positive delay; an integer line is the whole-sample cut bit for bit
    e, t = C.noise_pair(9000, 9000, 1, delay=17, noise=0.0)
    recs = score.drift_reference(e, t, 15.0, 0.0, 8)
    # (white noise: the side lobes of a block's own correlation, about 1 / sqrt(B) of the peak, tilt the parabola a little)
    assert len(recs) == 3 and all(r["d_int"] == 17 and r["k"] == 0 and r["flags"] == 0 and abs(r["tau"] - 17.0) < 1e-3 for r in recs)
    assert all(abs(r["rho"] - 1.0) < 1e-9 and r["z"] == 15 for r in recs)
    y, lo, hi = score.drift_warp_reference(e, len(t), 17.0, 0.0)
    ce, ct = score.align_cut(e, t, 17)
    assert (lo, hi) == (0, len(ce)) and C.same_f32(y, ce)
    y, lo, hi = score.drift_warp_reference(e, len(t), -5.0, 0.0)
    assert (lo, hi) == (5, 9000) and C.same_f32(y, e[:8995])
    # flags: the peak at the edge of the search, and a silent block
    assert all(r["flags"] & score.DRIFT_EDGE for r in score.drift_reference(e, t, 9.0, 0.0, 8))
    z = np.zeros(5000, np.float32)
    r = score.drift_reference(e[:5000], z, 0.0, 0.0, 4)[0]
    assert r["flags"] == score.DRIFT_SILENT and math.isnan(r["rho"]) and math.isnan(r["u"]) and r["d_int"] == 0 and r["tau"] == 0.0
    assert score.drift_reference(e[:4095], t[:4095]) == []
    with pytest.raises(ValueError):
        score.drift_reference(e, t, radius=1025)
    with pytest.raises(ValueError):
        score.drift_reference(e, t, cb=0.001)


def test_device_order_restated_stays_within_the_bars():
    """The order drift.hip states, restated on the host, against the reference: what the GPU test asks of the device is
    asked here of the restatement, so the bars are known to admit the stated order."""
    e, t = C.analytic_clip(C.B + 2 * C.H, 5.4, 300e-6, 30.0, 9)
    table = score.drift_table()
    worst = {}
    for R in (1, 8):
        for ref, bars, cbar in C.reference_segments(e, t, 6.0, 3e-4, R):
            got, c = C.device_order_segment(e, t, ref["u0"] // C.H, ref["z"], R, table)
            assert bars["decided"] > 1.0 and got["k"] == ref["k"]
            for k, v in C.segment_ratios(got, c, ref, bars, cbar).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("drift: the stated order against the reference, worst ratio to the bar", worst)
    assert max(worst.values()) <= 1.0, worst


def test_planted_faults_leave_their_bars():
    i = 1
    e, t = C.e2e_clip(i)
    n, a, b = C.E2E_CLIPS[i][:3]
    fit, refs, R, centre = C.reference_line(i)
    factors = {}
    # block centre in place of the centroid, and the hop off by one: the abscissae (and delays) against their bars
    wrong = C.fault_block_centre(refs)
    factors["block centre"] = min(C.ratio(w["u"], r[0]["u"], r[1]["u"]) for w, r in zip(wrong, refs))
    wrong = C.fault_hop_off_by_one(e, t, centre[0], centre[1], R)
    factors["hop off by one"] = min(max(C.ratio(w["u"], r[0]["u"], r[1]["u"]), C.ratio(w["tau"], r[0]["tau"], r[1]["tau"]))
                                    for w, r in list(zip(wrong, refs))[1:])
    # the warp: a wrong output against half a unit in the last place of the float32 output (the device is held bit for bit)
    table = score.drift_table()
    y, lo, hi = score.drift_warp_reference(e, n, fit["a"], fit["b"])
    half_ulp = 2.0 ** -24 * float(np.sqrt(np.mean(y.astype(np.float64) ** 2)))
    for name, kw in (("tap off by one", {"tap_shift": 1}), ("lambda dropped", {"drop_lambda": True})):
        w = C.fault_warp(e, n, fit["a"], fit["b"], table, **kw)
        factors[name] = float(np.sqrt(np.mean((w.astype(np.float64) - y) ** 2))) / half_ulp
    assert C.same_f32(C.fault_warp(e, n, fit["a"], fit["b"], table), y)
    print("drift planted faults: the fault's error over its bar", factors)
    assert min(factors.values()) > 1e3, factors
    # and what the centroid is for: the line fitted through block centres is off by far more than the fit's bar
    f2 = score.drift_fit(C.fault_block_centre(refs))
    bar_a, bar_b = C.fit_bar(refs)
    print("drift planted faults: the centre-fitted line moves a by %.3e (bar %.3e), b by %.3e (bar %.3e)"
          % (abs(f2["a"] - fit["a"]), bar_a, abs(f2["b"] - fit["b"]), bar_b))
    assert abs(f2["a"] - fit["a"]) > 1e3 * bar_a


def test_constants_match_the_kernel():
    k = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    m = re.search(r"kDriftFields = (\d+), kDriftFitFields = (\d+), kDriftT = (\d+), kDriftQ = (\d+), kDriftBlock = (\d+), kDriftHop = (\d+), "
                  r"kDriftMaxR = (\d+)", k)
    want = (hip.DRIFT_FIELDS, hip.DRIFT_FIT_FIELDS, hip.DRIFT_TAPS, hip.DRIFT_PHASES, hip.DRIFT_BLOCK, hip.DRIFT_HOP, hip.DRIFT_MAX_RADIUS)
    assert m and tuple(int(v) for v in m.groups()) == want == (8, 6, score.DRIFT_T, score.DRIFT_Q, score.DRIFT_BLOCK, score.DRIFT_HOP,
                                                               score.DRIFT_MAX_RADIUS)
    assert re.search(r"kDriftTile = (\d+)", k).group(1) == str(hip.DRIFT_TILE) == str(hip.ALIGN_TILE)
    assert re.search(r"kDriftFine = (\d+)", k).group(1) == str(hip.DRIFT_FINE) == str(score.DRIFT_FINE)
    assert re.search(r"kDriftWarpTile = (\d+)", k).group(1) == str(hip.DRIFT_WARP_TILE)
    assert float(re.search(r"kDriftMaxSlope = ([\d.]+)", k).group(1)) == score.DRIFT_MAX_SLOPE == 2.0 ** -10
    assert float(re.search(r"kDriftMaxDelay = ([\d.]+)", k).group(1)) == score.DRIFT_MAX_DELAY == 2.0 ** 31
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    for name, v in (("FIELDS", hip.DRIFT_FIELDS), ("FIT_FIELDS", hip.DRIFT_FIT_FIELDS), ("TAPS", hip.DRIFT_TAPS), ("PHASES", hip.DRIFT_PHASES),
                    ("BLOCK", hip.DRIFT_BLOCK), ("HOP", hip.DRIFT_HOP), ("MAX_RADIUS", hip.DRIFT_MAX_RADIUS)):
        assert re.search(r"#define NHANS_DRIFT_%s %d\b" % (name, v), header), name
    assert "#define NHANS_ABI_VERSION 5" in header and hip.ABI_VERSION == 5
    assert len(score.DRIFT_FIELDS) == hip.DRIFT_FIELDS and len(score.DRIFT_FIT_FIELDS) == hip.DRIFT_FIT_FIELDS
    names = re.search(r"^NAMES = (.*)$", open(os.path.join(ROOT, "n-hans_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "drift" in names and "host_drift" in names
    text = open(os.path.join(ROOT, "n-hans_amd", "csrc", "drift.hip")).read()
    assert "kDriftTile = 2,048" in text and "#pragma clang fp contract(off)" in text         # (the stated order names the tile)


def test_prototypes_and_signature_table_agree():
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    restypes = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    protos = (("nhans_drift_table", "int", 2), ("nhans_drift_segments", "int64_t", 1), ("nhans_drift_range", "int", 6),
              ("nhans_drift_fit", "int", 5), ("nhans_drift_track", "int", 12), ("nhans_drift_warp", "int", 10))
    for name, ret, nargs in protos:
        m = re.search(r"([A-Za-z_0-9]+)\s+%s\s*\(([^()]*)\)\s*;" % name, code)
        assert m and m.group(1) == ret and m.group(2).count(",") + 1 == nargs, name
        restype, argtypes = hip.SIGNATURES[name]
        assert restype is restypes[ret] and len(argtypes) == nargs, name
    order = list(hip.SIGNATURES)
    assert [n for n in order if n.startswith("nhans_drift_")] == [p[0] for p in protos]
    assert order.index("nhans_quality_tables") < order.index("nhans_drift_table") and order.index("nhans_drift_warp") < order.index("nhans_profile_json")
    assert code.index("nhans_quality_tables") < code.index("nhans_drift_table") < code.index("nhans_drift_warp") < code.index("nhans_profile_json")
    assert not [n for n in order if n.startswith("nhans_align") and "drift" in n]


def test_library_refuses_without_a_device(lib_built):
    C.check_refusals(hip.load(), None)

    class NoDevice(context.Context):
        pass

    with pytest.raises(ValueError, match="drift=True"):
        NoDevice().score([], [], drift=True)
    with pytest.raises(ValueError, match="drift=True"):
        NoDevice().score([np.zeros(4, np.float32)], [np.zeros(4, np.float32)], delays=[0], drift=True)


def test_cli_argument_errors(tmp_path):
    wav, tgt = str(tmp_path / "in.wav"), str(tmp_path / "t.wav")
    open(tgt, "wb").close()
    keys = ("input", "score_against", "align_ms", "align_drift")
    saved = {k: getattr(apply.FLAGS, k) for k in keys}
    try:
        for prog in ("nhans_denoiser", "nhans_separator"):
            a = apply._parse(["--input", wav, "--score_against", tgt, "--align_ms", "10", "--align_drift"], prog)
            assert a.align_drift is True and a.align_ms == 10.0
            assert apply._parse(["--input", wav, "--score_against", tgt, "--align_ms", "10"], prog).align_drift is False
            for argv in (["--input", wav, "--score_against", tgt, "--align_drift"], ["--input", wav, "--align_drift"]):
                with pytest.raises(SystemExit):
                    apply._parse(argv, prog)
    finally:
        for k, v in saved.items():
            setattr(apply.FLAGS, k, v)
