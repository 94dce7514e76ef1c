"""LLR, cepstral distance and fwSegSNR without a device: the float64 definition nhans_amd.score.quality_reference on known
answers and against independent formulations, the select's rule, the header's operation list on the host
(quality_checks.device_order_lpc) against the bars, the conditions every GPU test clip has to meet, the bars against
planted faults (each factor is printed: pytest -s), the kernel's constants, the header's prototypes, the refusals and the
command line's argument errors."""
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

import quality_checks as Q


def test_known_answers(lib_built):
    e, t = Q.clip(2000, 1)
    same = score.quality_reference(t, t, per_frame=True)
    assert (same["llr"], same["llr_95"], same["cd_db"], same["cd_95_db"], same["fwsegsnr_db"]) == (0.0, 0.0, 0.0, 0.0, 35.0)
    assert same["frames"] == same["frames_lpc"] == same["frames_fw"] == 13 and tuple(same)[:9] == score.QUALITY_FIELDS
    # a scaled copy: the LPC model does not see a gain -- 0 to the bar; fwSegSNR does: 20 log10(1 / 0.5) per band
    ref, bars = Q.reference_with_bars((0.5 * t).astype(np.float32), t)
    Q.conditions(ref, bars, exact=True)
    assert 0.0 <= ref["llr"] <= bars["llr"] and 0.0 <= ref["cd_db"] <= bars["cd_db"], (ref["llr"], bars["llr"], ref["cd_db"], bars["cd_db"])
    assert abs(ref["fwsegsnr_db"] - 20.0 * math.log10(2.0)) <= bars["fwsegsnr_db"]
    # counts and the empty clips
    for n, m in ((0, 0), (479, 0), (480, 1), (599, 1), (600, 2), (601, 2), (48000, 397)):
        assert score.quality_num_frames(n) == m
    r = score.quality_reference(e[:479], t[:479])
    assert r["frames"] == 0 and all(math.isnan(r[k]) for k in score.QUALITY_FIGURES)
    z = np.zeros(1000, np.float32)
    r = score.quality_reference(e[:1000], z, per_frame=True)
    assert r["frames"] == 5 and r["frames_lpc"] == r["frames_fw"] == 0 and np.isnan(r["per_frame"]).all()
    r = score.quality_reference(z, t[:1000])
    assert r["frames_lpc"] == 0 and r["frames_fw"] == 5 and abs(r["fwsegsnr_db"]) <= 35 * 4 * Q.U and math.isnan(r["llr"])       # (35 - 35 G / G: three roundings)
    rec = score.quality_record([7.0, 3.0, 2.0, 3.0, 0.5, 0.25, 1.5, 1.0, 12.0] + [0.0] * 7)
    assert rec == {"n": 7, "frames": 3, "frames_lpc": 2, "frames_fw": 3, "llr": 0.5, "llr_95": 0.25, "cd_db": 1.5, "cd_95_db": 1.0,
                   "fwsegsnr_db": 12.0}
    merged = score.merge_quality({"n": 9, "frames": 4, "snr_db": 1.0}, rec)
    assert merged["n"] == 9 and merged["quality_n"] == 7 and merged["quality_frames"] == 3 and merged["llr"] == 0.5
    imp = score.improvement(dict(rec, snr_db=1.0), dict(rec, snr_db=3.0, llr=0.25, cd_db=1.0, fwsegsnr_db=15.0))
    assert imp == {"snr_i": 2.0, "llr_i": -0.25, "llr_95_i": 0.0, "cd_i": -0.5, "cd_95_i": 0.0, "fwsegsnr_i": 3.0}


def test_ar2_closed_form_is_approached():
    """Target AR(2) with A_t = (1, -1.2, 0.6), estimate AR(2) with A_e = (1, -0.5, 0.3), unit innovations.  With the exact
    autocorrelation of the target, q(a) = a' R a and q(A_t) = 1: llr = ln(A_e' R A_e).  A frame of 480 windowed samples
    estimates sixteen coefficients from about 180 effective samples, which biases den down and num up by about 16 / 180
    each: a loose sanity bound, 0.47, twice the largest deviation of a clip's mean (22 frames) from the closed form 0.666
    that this reference showed over these 50 seeds (0.235) -- not a device figure."""
    rho1 = 1.2 / (1.0 + 0.6)
    r0 = 1.0 / (1.0 - 1.2 * rho1 + 0.6 * (1.2 * rho1 - 0.6))
    r = [r0, rho1 * r0, (1.2 * rho1 - 0.6) * r0]
    Ae = np.array([1.0, -0.5, 0.3])
    closed = math.log(float(Ae @ score.quality_toeplitz(r) @ Ae))
    worst = 0.0
    for seed in range(50):
        t = Q.coloured(3000, 100 + seed).astype(np.float32)
        e = Q.coloured(3000, 900 + seed, poles=(0.5, -0.3)).astype(np.float32)
        worst = max(worst, abs(score.quality_reference(e, t)["llr"] - closed))
    print("quality AR(2): closed form %.4f, worst deviation of a clip's mean over 50 seeds %.4f" % (closed, worst))
    assert worst < 0.47


def test_reference_against_an_independent_formulation(lib_built):
    e, t = Q.clip(1320, 2)
    ref = score.quality_reference(e, t, per_frame=True, details=True)
    w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 1) / 481.0) for i in range(480)])
    assert Q.same_bits(score.quality_window(), w)
    te, tt = e.astype(np.float64), t.astype(np.float64)
    for f in (0, 3, 7):
        d = ref["lpc"][f]
        xs = [tt[120 * f:120 * f + 480] * w, te[120 * f:120 * f + 480] * w]
        r = [np.array([np.dot(x[:480 - k], x[k:]) for k in range(17)]) for x in xs]
        # LPC by a dense solve of the Toeplitz system
        a = [np.concatenate([[1.0], np.linalg.solve(score.quality_toeplitz(v[:16]), -v[1:])]) for v in r]
        cond = max(np.linalg.cond(score.quality_toeplitz(v)) for v in r)
        assert np.abs(a[0] - d["a_t"]).max() <= Q.C_A * Q.U * cond * np.linalg.norm(a[0])
        assert np.abs(a[1] - d["a_e"]).max() <= Q.C_A * Q.U * cond * np.linalg.norm(a[1])
        llr = math.log((a[1] @ score.quality_toeplitz(r[0]) @ a[1]) / (a[0] @ score.quality_toeplitz(r[0]) @ a[0]))
        assert abs(llr - ref["per_frame"][f, 0]) <= Q.lpc_bars(d)["llr"]
        # the cepstrum as the transform of -ln |A| on 4,096 points: c[m] aliases with c[m + 4096 j], and |c[m]| <= 16 rho^m / m
        # with rho the largest pole radius
        cs = []
        for aa in a:
            A = np.fft.fft(aa, 4096)
            c = np.fft.ifft(-np.log(A)).real
            rho = np.abs(np.roots(aa)).max()
            assert rho < 1.0
            cs.append(c[:17])
            assert np.abs(c[1:17] - score.quality_cepstrum(aa)[1:]).max() <= 2 * 16 * rho ** 4096 / 4096 / (1 - rho ** 4096) + 1e-12
        cd = score.QUALITY_CD_SCALE * math.sqrt(2.0 * float(((cs[0] - cs[1])[1:] ** 2).sum()))
        assert abs(cd - ref["per_frame"][f, 1]) <= 1e-9
    # fwSegSNR by a direct DFT of one frame
    f = 5
    k = np.arange(257)[:, None] * np.arange(480)[None, :]
    Fm = np.exp(-2j * np.pi * k / 512.0)
    W = score.quality_band_matrix()
    X, Y = W @ np.abs(Fm @ (tt[120 * f:120 * f + 480] * w)), W @ np.abs(Fm @ (te[120 * f:120 * f + 480] * w))
    s = np.clip(10 * np.log10(X ** 2 / (X - Y) ** 2), -10, 35)
    assert abs(float((X ** 0.2 * s).sum() / (X ** 0.2).sum()) - ref["per_frame"][f, 2]) <= 1e-9
    # the default band matrix: 25 triangles that tile the mel axis, built independently
    mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
    p = 700.0 * (10.0 ** (np.linspace(mel(0.0), mel(8000.0), 27) / 2595.0) - 1.0)
    fr = 31.25 * np.arange(257)
    want = np.array([np.maximum(0.0, np.minimum((fr - p[m]) / (p[m + 1] - p[m]), (p[m + 2] - fr) / (p[m + 2] - p[m + 1]))) for m in range(25)])
    assert W.shape == (25, 257) and np.abs(W - want).max() <= 1e-12 and (W.sum(axis=1) > 0).all() and (W >= 0).all()


def test_the_selects_rule():
    """q = (19 Mk + 10) // 20 in exact rational arithmetic is round-half-up of 0.95 Mk; the trimmed mean with ties at the
    threshold equals the device's form (sum below + (q - count below) v) / q."""
    rng = np.random.default_rng(4)
    for mk in range(1, 42):
        q = (19 * mk + 10) // 20
        assert q == math.floor(fractions.Fraction(19 * mk, 20) + fractions.Fraction(1, 2)) and 1 <= q <= mk
        v = np.round(rng.random(mk) * 4) / 4            # quarters: many ties, every sum exact
        got = score.quality_trimmed_mean(v.tolist())
        s = sorted(v.tolist())
        thr = s[q - 1]
        below = [x for x in v.tolist() if x < thr]
        assert got == (sum(below) + (q - len(below)) * thr) / q == float(sum(fractions.Fraction(x) for x in s[:q]) / q)
    assert [(19 * m + 10) // 20 for m in (1, 10, 11, 30)] == [1, 10, 10, 29]
    assert math.isnan(score.quality_trimmed_mean([]))


def test_device_order_on_the_host_is_within_the_bars(lib_built):
    """The header's operation list, repeated on the host, against the definition: every quantity within its bar, and far
    inside it."""
    e, t = Q.clip(1320, 3)
    ref, bars = Q.reference_with_bars(e, t)
    Q.conditions(ref, bars)
    rows = Q.device_order_lpc(e, t)
    worst = {"r": 0.0, "llr": 0.0, "cd": 0.0}
    for f in range(ref["frames"]):
        d, b = ref["lpc"][f], bars["lpc"][f]
        worst["r"] = max(worst["r"], np.abs(rows[f, :17] - d["r_t"]).max() / b["r"][0], np.abs(rows[f, 17:34] - d["r_e"]).max() / b["r"][1])
        num, den, dc2 = rows[f, 68:71]
        worst["llr"] = max(worst["llr"], abs(math.log(num / den) - ref["per_frame"][f, 0]) / b["llr"])
        worst["cd"] = max(worst["cd"], abs(score.QUALITY_CD_SCALE * math.sqrt(2 * dc2) - ref["per_frame"][f, 1]) / b["cd"])
        assert rows[f, 34] == 1.0 and rows[f, 51] == 1.0 and rows[f, 71] == 0.0
    print("quality host: the device's order against the definition, worst ratio to the bar", worst)
    assert max(worst.values()) <= 1.0


def test_every_gpu_clip_meets_the_conditions(lib_built):
    """cond2(R) <= 1e8 on every kept frame of every clip the GPU tests use, and no value within twice its bar of a clamp edge
    or of the select's threshold."""
    worst = 0.0
    full = Q.reference_with_bars(*Q.base_clip())
    for n in [s for s in Q.SIZES if s >= 480]:
        ref, bars = Q.prefix(*full, n)
        assert ref["frames_lpc"] == ref["frames"] == score.quality_num_frames(n) and ref["n"] == n
        worst = max(worst, Q.conditions(ref, bars))
    e, t = Q.base_clip()
    alone = score.quality_reference(e[:1321], t[:1321], per_frame=True)
    cut, _ = Q.prefix(*full, 1321)
    assert all(float(alone[k]).hex() == float(cut[k]).hex() for k in score.QUALITY_FIELDS) and Q.same_bits(alone["per_frame"], cut["per_frame"])
    ref, bars = Q.reference_with_bars(*Q.clip(Q.LONG, 12))
    worst = max(worst, Q.conditions(ref, bars))
    for e, t in (Q.periodic_clip(), Q.zero_runs_clip()):
        ref, bars = Q.reference_with_bars(e, t)
        worst = max(worst, Q.conditions(ref, bars, exact=True))
    e, t = Q.zero_runs_clip()
    ref = score.quality_reference(e, t, per_frame=True)
    skipped = np.isnan(ref["per_frame"])
    assert skipped[:4, :].all() and skipped[-4:, :].all()                       # leading (target) and trailing (both) runs
    assert skipped[17:21, 0].all() and not skipped[17:21, 2].any()              # inner run of the estimate: fw is 0 dB there
    assert 0 < ref["frames_lpc"] < ref["frames_fw"] < ref["frames"]
    print("quality clips: largest cond2(R) of a kept frame %.3g (<= %.0e)" % (worst, Q.COND_MAX))


def test_the_bars_see_the_planted_faults(lib_built):
    e, t = Q.clip(1320, 6)
    ref, bars = Q.reference_with_bars(e, t)
    factors = {}
    for fault in Q.FAULTS:
        per, rows = Q.faulty_reference(e, t, fault)
        worst = 0.0
        for f in range(ref["frames"]):
            d, b = ref["lpc"][f], bars["lpc"][f]
            got = [abs(per[f, 0] - ref["per_frame"][f, 0]) / b["llr"], abs(per[f, 1] - ref["per_frame"][f, 1]) / b["cd"],
                   np.abs(rows[f, :17] - d["r_t"]).max() / b["r"][0], np.abs(rows[f, 17:] - d["r_e"]).max() / b["r"][1]]
            worst = max([worst] + [v for v in got if v == v])
        factors[fault] = float(worst)
    print("quality planted faults: worst error over its bar", factors)
    assert len(factors) >= 4 and min(factors.values()) > 1e6, factors


def test_constants_match_the_kernel():
    k = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    m = re.search(r"kQualityFields = (\d+), kQualityFrame = (\d+), kQualityHop = (\d+), kQualityOrder = (\d+), kQualityFft = (\d+), kQualityBins = (\d+)", k)
    want = (hip.QUALITY_FIELDS, hip.QUALITY_FRAME, hip.QUALITY_HOP, hip.QUALITY_ORDER, hip.QUALITY_FFT, hip.QUALITY_BINS)
    assert m and tuple(int(v) for v in m.groups()) == want == (16, score.QUALITY_FRAME, score.QUALITY_HOP, score.QUALITY_ORDER, score.QUALITY_FFT, score.QUALITY_BINS)
    m = re.search(r"kQualityBands = (\d+), kQualityMaxBands = (\d+), kQualityLpcTile = (\d+), kQualityBandTile = (\d+)", k)
    assert m and tuple(int(v) for v in m.groups()) == (hip.QUALITY_BANDS, hip.QUALITY_MAX_BANDS, Q.LT, Q.BT) == (score.QUALITY_BANDS, score.QUALITY_MAX_BANDS, 7, 2)
    assert re.search(r"kQualityLpcFields = (\d+)", k).group(1) == str(hip.QUALITY_LPC_FIELDS) == str(4 * 17 + 4)
    m = re.search(r"kQualityLlrMax = ([\d.]+), kQualityCdMax = ([\d.]+), kQualityCdScale = ([\d.]+)", k)
    assert tuple(float(v) for v in m.groups()) == (score.QUALITY_LLR_MAX, score.QUALITY_CD_MAX, score.QUALITY_CD_SCALE)
    assert abs(score.QUALITY_CD_SCALE - 10.0 / math.log(10.0)) <= 1e-15
    m = re.search(r"kQualitySnrMin = (-?[\d.]+), kQualitySnrMax = ([\d.]+), kQualityGamma = ([\d.]+)", k)
    assert tuple(float(v) for v in m.groups()) == (score.QUALITY_SNR_MIN, score.QUALITY_SNR_MAX, score.QUALITY_GAMMA)
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    for name, v in (("FIELDS", hip.QUALITY_FIELDS), ("LPC_FIELDS", hip.QUALITY_LPC_FIELDS), ("BINS", hip.QUALITY_BINS),
                    ("BANDS", hip.QUALITY_BANDS), ("MAX_BANDS", hip.QUALITY_MAX_BANDS)):
        assert re.search(r"#define NHANS_QUALITY_%s %d\b" % (name, v), header), name
    assert "#define NHANS_ABI_VERSION 5" in header and hip.ABI_VERSION == 5
    assert len(score.QUALITY_FIELDS) == 9 and score.QUALITY_FIGURES == ("llr", "llr_95", "cd_db", "cd_95_db", "fwsegsnr_db")
    names = re.search(r"^NAMES = (.*)$", open(os.path.join(ROOT, "n-hans_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "quality" in names and "host_quality" in names


def test_prototypes_and_signature_table_agree():
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name, nargs in (("nhans_quality", 11), ("nhans_quality_lpc", 8), ("nhans_quality_tables", 2)):
        m = re.search(r"([A-Za-z_0-9]+)\s+%s\s*\(([^()]*)\)\s*;" % name, code)
        assert m and m.group(1) == "int" and m.group(2).count(",") + 1 == nargs, name
        restype, argtypes = hip.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    order = list(hip.SIGNATURES)
    assert order.index("nhans_align_cut") < order.index("nhans_quality") < order.index("nhans_profile_json")
    assert code.index("nhans_align_cut") < code.index("nhans_quality(") < code.index("nhans_profile_json")


def test_library_refuses_without_a_device(lib_built):
    Q.check_refusals(hip.load(), None)
    with pytest.raises(ValueError):
        score.quality_reference(np.zeros(600, np.float32), np.zeros(600, np.float32), bands=-np.ones((1, 257)))
    with pytest.raises(ValueError):
        score.quality_reference(np.zeros(600, np.float32), np.zeros(600, np.float32), bands=np.ones((33, 257)))


def test_cli_argument_errors(tmp_path):
    wav, tgt = str(tmp_path / "in.wav"), str(tmp_path / "t.wav")
    open(tgt, "wb").close()
    keys = ("input", "score_against", "quality")
    saved = {k: getattr(apply.FLAGS, k) for k in keys}
    try:
        for prog in ("nhans_denoiser", "nhans_separator"):
            assert apply._parse(["--input", wav, "--score_against", tgt, "--quality"], prog).quality is True
            assert apply._parse(["--input", wav, "--score_against", tgt], prog).quality is False
            with pytest.raises(SystemExit):
                apply._parse(["--input", wav, "--quality"], prog)
    finally:
        for k, v in saved.items():
            setattr(apply.FLAGS, k, v)
