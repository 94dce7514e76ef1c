"""Scoring against a clean target, the host side: the C ABI's surface and refusals, the float64 definition on pairs that
can be computed by hand, the fixture, the command line's refusals, and the bar's sight of planted faults
(tests/score_checks.py).  The device side: tests/test_gpu_score.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, score

import score_checks as S


# ------------------------------------------------------------------------------ surface
def test_header_table_and_field_counts(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    assert int(re.search(r"#define NHANS_SCORE_FIELDS (\d+)", header).group(1)) == hip.SCORE_FIELDS == 16
    assert int(re.search(r"#define NHANS_SCORE_ROW_FIELDS (\d+)", header).group(1)) == hip.SCORE_ROW_FIELDS == 8
    assert len(score.FIELDS) == 12 and len(score.ROW_FIELDS) == 3           # the rest of a record is zero
    assert len(hip.SIGNATURES["nhans_score_wave"][1]) == 9 and len(hip.SIGNATURES["nhans_score_rows"][1]) == 8
    kernels = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    assert "kScoreTile = %d" % hip.SCORE_TILE in kernels and "kScoreFields = 16" in kernels and "kScoreRowFields = 8" in kernels
    assert hip.SCORE_TILE % 80 == 0 and 400 % 80 == 0 and 160 % 80 == 0     # frames are whole segments
    lib = hip.load()
    assert lib.nhans_abi_version() == 5
    assert hasattr(lib, "nhans_score_wave") and hasattr(lib, "nhans_score_rows")


def test_refusals_before_the_device_is_touched(lib_built):
    """Every argument check comes before the context is looked at: a NULL context is only reported for a call that has
    nothing else wrong."""
    lib = hip.load()
    buf = ctypes.c_void_p(4096)            # a pointer that is never followed
    off = hip.i64_array

    def err():
        return lib.nhans_last_error().decode()

    assert lib.nhans_score_wave(None, buf, off([0, 10]), buf, off([0, 10]), -1, buf, None, None) == -1 and "negative clip count" in err()
    assert lib.nhans_score_wave(None, buf, None, buf, off([0, 10]), 1, buf, None, None) == -1 and "null" in err()
    assert lib.nhans_score_wave(None, buf, off([0, 10]), buf, off([0, 10]), 1, None, None, None) == -1 and "null" in err()
    assert lib.nhans_score_wave(None, buf, off([0, 10, 5]), buf, off([0, 10, 20]), 2, buf, None, None) == -1
    assert "clip 1" in err() and "estimate offsets descend" in err()
    assert lib.nhans_score_wave(None, buf, off([0, 10, 20]), buf, off([7, 3, 20]), 2, buf, None, None) == -1
    assert "clip 0" in err() and "target offsets descend" in err()
    assert lib.nhans_score_wave(None, None, off([0, 0, 10]), buf, off([0, 5, 20]), 2, buf, None, None) == -1
    assert "clip 1" in err() and "null buffer" in err()
    # nothing wrong but the context: a clip of no samples needs no buffer
    assert lib.nhans_score_wave(None, None, off([0, 0]), None, off([0, 5]), 1, buf, None, None) == -1 and "null context" in err()
    assert lib.nhans_score_wave(None, None, None, None, None, 0, None, None, None) == -1 and "null context" in err()

    assert lib.nhans_score_rows(None, buf, buf, off([0, 3]), -2, buf, None, None) == -1 and "negative clip count" in err()
    assert lib.nhans_score_rows(None, buf, buf, None, 1, buf, None, None) == -1 and "null" in err()
    assert lib.nhans_score_rows(None, buf, buf, off([0, 3, 2]), 2, buf, None, None) == -1
    assert "clip 1" in err() and "frame offsets descend" in err()
    assert lib.nhans_score_rows(None, buf, None, off([0, 0, 2]), 2, buf, None, None) == -1
    assert "clip 1" in err() and "null buffer" in err()
    assert lib.nhans_score_rows(None, None, None, off([0, 0]), 1, buf, None, None) == -1 and "null context" in err()


# ------------------------------------------------------------------------------ the definition, by hand
def test_reference_on_hand_computable_pairs():
    t = np.array([0.5, -0.25, 1.0, 0.125] * 100, dtype=np.float32)                  # 400 samples: one frame
    r = score.reference(t, t)
    assert r["alpha"] == 1.0 and r["Srr"] == 0.0 and r["Sdd"] == 0.0
    assert r["si_sdr_db"] == math.inf and r["snr_db"] == math.inf
    assert (r["segsnr_db"], r["frames_counted"], r["frames_skipped"]) == (35.0, 1, 0)
    assert r["Stt"] == 100 * (0.25 + 0.0625 + 1.0 + 0.015625) and r["n"] == 400
    r = score.reference(2 * t, t)
    assert r["alpha"] == 2.0 and r["Srr"] == 0.0 and r["si_sdr_db"] == math.inf
    assert r["snr_db"] == 0.0 and r["segsnr_db"] == 0.0 and r["Sdd"] == r["Stt"]
    # orthogonal: e = (1, 1, ...), t = (1, -1, ...): alpha = 0, all of e is distortion
    e, t2 = np.ones(400, np.float32), np.tile(np.array([1.0, -1.0], np.float32), 200)
    r = score.reference(e, t2)
    assert r["Set"] == 0.0 and r["alpha"] == 0.0 and r["Srr"] == 400.0 and r["si_sdr_db"] == -math.inf
    assert r["snr_db"] == pytest.approx(10 * math.log10(400.0 / 800.0), abs=1e-13)
    # silent target
    r = score.reference(e, np.zeros(400, np.float32))
    assert r["alpha"] == 0.0 and math.isnan(r["snr_db"]) and math.isnan(r["si_sdr_db"]) and math.isnan(r["segsnr_db"])
    assert (r["frames_counted"], r["frames_skipped"]) == (0, 1)
    # nothing at all, and the common prefix
    r = score.reference(np.zeros(0, np.float32), np.zeros(5, np.float32))
    assert r["n"] == 0 and r["See"] == 0.0 and math.isnan(r["snr_db"]) and math.isnan(r["segsnr_db"])
    assert score.reference(np.concatenate([t, e]), t) == score.reference(t, t)
    # a non-finite sample propagates
    bad = t.copy()
    bad[7] = np.inf
    assert math.isnan(score.reference(bad, t)["snr_db"]) or score.reference(bad, t)["snr_db"] == -math.inf
    # a frame at each clamp, a skipped one and a perfect one
    e, t3 = S.clamp_clip()
    seg, skipped = score.frame_snr(e, t3)
    assert seg[0] == -10.0 and seg[5] == 35.0 and not skipped.any()
    raw = score.frame_snr(e, t3, lo=-math.inf, hi=math.inf)[0]
    # (100 t is rounded to float32: 2^-24 relative on e, 20 / ln 10 x 100 / 99 x 2^-24 = 5.2e-7 dB)
    assert raw[0] == pytest.approx(-20 * math.log10(99.0), abs=1e-6) and raw[5] > 60.0
    e, t4 = S.silent_frames_clip()
    r = score.reference(e, t4, frames=True)
    assert (r["frames_counted"], r["frames_skipped"]) == (8, 3) and np.isnan(r["frames"][2:5]).all()
    assert (r["frames"][8:] == 35.0).all() and np.isfinite(r["frames"][[0, 1, 5, 6, 7]]).all()
    # rows: a constant difference of 1 -> loss = mean(imp) = 1.5, lsd = 20 / ln 10
    E, T = np.ones((3, 201), np.float32), np.zeros((3, 201), np.float32)
    r = score.reference_rows(E, T)
    assert r["loss"] == pytest.approx(1.5, abs=1e-7) and r["lsd_db"] == pytest.approx(20 / math.log(10), rel=1e-15)
    assert math.isnan(score.reference_rows(E[:0], T[:0])["loss"])
    imp = score.improvement({"si_sdr_db": 2.0, "snr_db": 3.0, "segsnr_db": -1.0, "loss": 6.0},
                            {"si_sdr_db": 7.0, "snr_db": 8.5, "segsnr_db": 5.0, "loss": 1.5})
    assert imp == {"si_sdr_i": 5.0, "snr_i": 5.5, "segsnr_i": 6.0, "loss_ratio": 0.25}


def test_fma_of_the_reference_is_exact_where_it_matters():
    """r = fma(-alpha, t, e) without a fused operation in numpy: against exact rational arithmetic."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    t = rng.standard_normal(64).astype(np.float32).astype(np.float64)
    alpha = 0.9371532981234567
    e = (alpha * t * (1.0 + 1e-9 * rng.standard_normal(64))).astype(np.float32).astype(np.float64)
    r = score._fma_neg(alpha, t, e)
    for i in range(64):
        exact = Fraction(e[i]) - Fraction(alpha) * Fraction(t[i])
        assert abs(Fraction(r[i]) - exact) <= abs(exact) * Fraction(1, 2 ** 52)


# ------------------------------------------------------------------------------ the fixture
def test_fixture_reproduces_and_denoised_beats_mixed():
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "score_demo_pairs.npz")) < (1 << 20)
    keys = [str(k) for k in g["score_keys"]]
    assert keys == list(score.FIELDS) + ["loss", "lsd_db"]
    for ex, n in (("example2", 22480), ("example3", 28080)):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        assert all(v.dtype == np.float32 and v.shape == (n,) for v in sig.values())
        rec = {}
        for k in ("mixed", "denoised"):
            rec[k] = dict(zip(keys, g["%s_%s_scores" % (ex, k)]))
            again = score.reference_all(sig[k], sig["target"])
            assert all(again[name] == rec[k][name] for name in keys), (ex, k)
            assert rec[k]["frames_skipped"] == 0                        # no silent target frame
        for fig in ("si_sdr_db", "snr_db", "segsnr_db"):
            assert rec["denoised"][fig] > rec["mixed"][fig], (ex, fig)
        for fig in ("loss", "lsd_db"):
            assert rec["denoised"][fig] < rec["mixed"][fig], (ex, fig)
        imp = score.improvement(rec["mixed"], rec["denoised"])
        assert imp["si_sdr_i"] > 2.5 and imp["snr_i"] > 2.5 and imp["segsnr_i"] > 5.0 and imp["loss_ratio"] < 0.25


# ------------------------------------------------------------------------------ command line
def test_cli_refuses_what_it_cannot_score(tmp_path, capsys):
    from scipy.io import wavfile
    ind, tgd = tmp_path / "in", tmp_path / "tgt"
    ind.mkdir()
    tgd.mkdir()
    for name in ("a.wav", "b.wav"):
        wavfile.write(str(ind / name), 16000, np.zeros(800, np.int16))
    wavfile.write(str(tgd / "a.wav"), 16000, np.zeros(800, np.int16))
    one, tone = str(ind / "a.wav"), str(tgd / "a.wav")

    def refused(argv, *words):
        with pytest.raises(SystemExit):
            apply._parse(argv, "nhans_denoiser")
        msg = capsys.readouterr().err
        assert all(w in msg for w in words), msg

    try:
        refused(["--input", one, "--score_against", tone, "--output_rate", "input"], "--output_rate input")
        refused(["--input", one, "--score_against", tone, "--convert_on", "gpu"], "--convert_on gpu")
        refused(["--input", str(ind), "--output", str(tmp_path / "o"), "--score_against", str(tgd)], "b.wav", "no target")
        refused(["--input", str(ind), "--output", str(tmp_path / "o"), "--score_against", tone], "directory")
        refused(["--input", one, "--score_against", str(tgd)], "directory")
        refused(["--input", one, "--score_against", str(tmp_path / "missing.wav")], "not a file")
        refused(["--input", one, "--score_out", str(tmp_path / "s.json")], "--score_against")
        a = apply._parse(["--input", one, "--score_against", tone, "--score_out", str(tmp_path / "s.json")], "nhans_separator")
        assert (a.score_against, a.score_out) == (tone, str(tmp_path / "s.json"))
        assert apply._parse(["--input", one], "nhans_denoiser").score_against is None
    finally:
        for k in ("score_against", "score_out"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.output_rate, apply.FLAGS.convert_on = "16000", "host"
        apply.FLAGS.input, apply.FLAGS.output = apply.Flags.input, apply.Flags.output


def test_target_is_put_on_the_inputs_scale(tmp_path):
    from scipy.io import wavfile
    x = np.array([100, -2000, 500, 1000], dtype=np.int16)
    t = np.array([50, -1000, 250, 7], dtype=np.int16)
    wavfile.write(str(tmp_path / "x.wav"), 16000, x)
    wavfile.write(str(tmp_path / "t.wav"), 16000, t)
    got = apply.scaled_target(str(tmp_path / "x.wav"), str(tmp_path / "t.wav"))
    assert got.dtype == np.float32 and np.array_equal(got, (t / (2000 + 0.000001)).astype(np.float32))
    assert np.array_equal(apply.normalise(x), (x / (2000 + 0.000001)).astype(np.float32))      # the input's own factor


# ------------------------------------------------------------------------------ the bar sees planted faults
def test_the_bar_passes_the_reference_and_sees_planted_faults():
    e, t = S.clip(2 * S.TILE + 1, 5)
    ref = score.reference(e, t, frames=True)
    assert max(S.wave_ratios(ref, e, t).values()) == 0.0
    # a sum in another order (numpy's pairwise float64 sum) is inside the bar, comfortably
    other = dict(ref)
    e64, t64 = e.astype(np.float64), t.astype(np.float64)
    other.update(See=float(np.sum(e64 * e64)), Stt=float(np.sum(t64 * t64)), Sdd=float(np.sum((e64 - t64) ** 2)))
    r = S.wave_ratios(other, e, t)
    assert 0.0 < max(r["See"], r["Stt"], r["Sdd"]) < 0.5
    WIDE = 1e6
    got = S.fault_dropped_last_sample(e, t)
    got["n"] += 1                                                       # (the count itself would already give it away)
    r = S.wave_ratios(got, e, t)
    assert min(r[k] for k in ("See", "Stt", "Sdd", "Srr", "snr_db", "si_sdr_db")) > WIDE, r
    r = S.wave_ratios(S.fault_frame_count_off_by_one(e, t), e, t)
    assert r["segsnr_db"] > WIDE and r["snr_db"] == 0.0
    ec, tc = S.clamp_clip()
    r = S.wave_ratios(S.fault_clamp_after_mean(ec, tc), ec, tc)
    assert r["segsnr_db"] > WIDE, r
    E, T = S.uniform_rows(17, 1), S.uniform_rows(17, 2)
    assert max(S.rows_ratios(score.reference_rows(E, T, frames=True), E, T).values()) == 0.0
    r = S.rows_ratios(S.fault_imp_reversed(E, T), E, T)
    assert r["loss"] > WIDE and r["lsd_db"] == 0.0, r
