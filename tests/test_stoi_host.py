"""STOI and extended STOI, the host side: the C ABI's surface and refusals, the band table from its formula, the float64
definition on pairs that can be checked by hand, the two conditions that keep the bar honest on every test clip, the
command line's refusal, and the bar's sight of planted faults (tests/stoi_checks.py).  The device side:
tests/test_gpu_stoi.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, score

import stoi_checks as S

NAMES = ["nhans_stoi_out_count", "nhans_stoi_resample", "nhans_stoi"]


# ------------------------------------------------------------------------------ surface
def test_header_table_and_signatures_agree(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    assert int(re.search(r"#define NHANS_STOI_FIELDS (\d+)", header).group(1)) == hip.STOI_FIELDS == 8
    assert len(score.STOI_FIELDS) == 6                                                     # the rest of a record is zero
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    names = re.findall(r"\b(nhans_[a-z_0-9]+)\s*\(", code)
    assert [n for n in names if n.startswith("nhans_stoi")] == NAMES == [n for n in hip.EXPORTS if n.startswith("nhans_stoi")]
    assert names.index("nhans_mix") < min(names.index(n) for n in NAMES)
    assert max(names.index(n) for n in NAMES) < names.index("nhans_profile_json")
    assert [len(hip.SIGNATURES[n][1]) for n in NAMES] == [1, 7, 9]
    assert hip.SIGNATURES["nhans_stoi_out_count"][0] is ctypes.c_int64
    kernels = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    assert "kStoiFields = 8" in kernels and "kStoiBands = 15" in kernels and "kStoiSegment = 30" in kernels
    # the kernel's band edges are the table's
    src = open(os.path.join(ROOT, "n-hans_amd", "csrc", "stoi.hip")).read()
    edges = [int(v) for v in re.search(r"kBandEdge\[kStoiBands \+ 1\] = \{([^}]*)\}", src).group(1).split(",")]
    assert edges == [lo for lo, _ in score.STOI_BANDS] + [score.STOI_BANDS[-1][1]]
    assert float(re.search(r"kStoiClip = ([0-9.e+-]+);", src).group(1)) == score.STOI_CLIP
    assert float(re.search(r"kStoiEps = ([0-9.e+-]+);", src).group(1)) == score.STOI_EPS == 2.0 ** -52
    lib = hip.load()
    assert lib.nhans_abi_version() == 5 and re.search(r"#define NHANS_ABI_VERSION 5\b", header)
    assert all(hasattr(lib, n) for n in NAMES)
    # the public list of rate pairs is what it was: 10 kHz is not one of them
    assert lib.nhans_resample_out_count(100, 16000, 10000) == -1 and b"not supported" in lib.nhans_last_error()


def test_out_count(lib_built):
    lib = hip.load()
    for n in (0, 1, 7, 8, 9, 6555):
        assert lib.nhans_stoi_out_count(n) == -((-5 * n) // 8) == score.stoi_out_count(n) == math.ceil(5 * n / 8)
    assert [score.stoi_out_count(n) for n in (0, 1, 7, 8, 9, 6555)] == [0, 1, 5, 5, 6, 4097]
    assert lib.nhans_stoi_out_count(-1) == -1 and b"negative" in lib.nhans_last_error()


def test_refusals_before_the_device_is_touched(lib_built):
    """Every argument check comes before the context is looked at: a NULL context is only reported for a call that has
    nothing else wrong."""
    lib = hip.load()
    buf = ctypes.c_void_p(4096)            # a pointer that is never followed
    off = hip.i64_array

    def err():
        return lib.nhans_last_error().decode()

    assert lib.nhans_stoi(None, buf, off([0, 10]), buf, off([0, 10]), -1, buf, None, None) == -1 and "negative clip count" in err()
    assert lib.nhans_stoi(None, buf, None, buf, off([0, 10]), 1, buf, None, None) == -1 and "null" in err()
    assert lib.nhans_stoi(None, buf, off([0, 10]), buf, off([0, 10]), 1, None, None, None) == -1 and "null" in err()
    assert lib.nhans_stoi(None, buf, off([0, 10, 5]), buf, off([0, 10, 20]), 2, buf, None, None) == -1
    assert "clip 1" in err() and "estimate offsets descend" in err()
    assert lib.nhans_stoi(None, buf, off([0, 10, 20]), buf, off([7, 3, 20]), 2, buf, None, None) == -1
    assert "clip 0" in err() and "target offsets descend" in err()
    assert lib.nhans_stoi(None, None, off([0, 0, 10]), buf, off([0, 5, 20]), 2, buf, None, None) == -1
    assert "clip 1" in err() and "null buffer" in err()
    # nothing wrong but the context: a clip of no samples needs no buffer
    assert lib.nhans_stoi(None, None, off([0, 0]), None, off([0, 5]), 1, buf, None, None) == -1 and "null context" in err()
    assert lib.nhans_stoi(None, None, None, None, None, 0, None, None, None) == -1 and "null context" in err()

    assert lib.nhans_stoi_resample(None, buf, off([0, 8]), -3, buf, off([0, 5]), None) == -1 and "negative clip count" in err()
    assert lib.nhans_stoi_resample(None, buf, None, 1, buf, off([0, 5]), None) == -1 and "null" in err()
    assert lib.nhans_stoi_resample(None, buf, off([0, 8]), 1, buf, None, None) == -1 and "null" in err()
    assert lib.nhans_stoi_resample(None, buf, off([0, 8, 4]), 2, buf, off([0, 5, 10]), None) == -1
    assert "clip 1" in err() and "input offsets descend" in err()
    assert lib.nhans_stoi_resample(None, buf, off([0, 8, 16]), 2, buf, off([5, 0, 10]), None) == -1
    assert "clip 0" in err() and "output offsets descend" in err()
    assert lib.nhans_stoi_resample(None, buf, off([0, 8, 17]), 2, buf, off([0, 5, 10]), None) == -1
    assert "clip 1" in err() and "5 samples, 6 needed" in err()
    assert lib.nhans_stoi_resample(None, None, off([0, 0, 8]), 2, buf, off([0, 0, 5]), None) == -1
    assert "clip 1" in err() and "null buffer" in err()
    assert lib.nhans_stoi_resample(None, None, off([0, 0]), 1, None, off([0, 0]), None) == -1 and "null context" in err()
    assert lib.nhans_stoi_resample(None, None, None, 0, None, None, None) == -1 and "null context" in err()


# ------------------------------------------------------------------------------ the definition
def test_band_table_from_its_formula():
    assert score.stoi_band_table() == score.STOI_BANDS and len(score.STOI_BANDS) == 15
    assert all(a[1] == b[0] for a, b in zip(score.STOI_BANDS, score.STOI_BANDS[1:]))        # contiguous
    w = score.stoi_window()
    assert len(w) == 256 and np.allclose(w, np.hanning(258)[1:-1], rtol=0, atol=1e-15) and w[0] > 0.0
    assert score.STOI_CLIP == 1.0 + 10.0 ** 0.75


def test_framing_by_the_published_rule():
    for n, m in ((0, 0), (256, 0), (257, 1), (384, 1), (385, 2), (4096, 30), (4097, 31), (4224, 31), (4225, 32)):
        assert score.stoi_num_frames(n) == m == len(score.stoi_frames(np.zeros(n), score.stoi_window()))
    # the rejoined signal of Mk frames gives Mk - 1 frames
    for mk in (0, 1, 2, 31):
        j = score.stoi_rejoin(np.ones((mk, 256)))
        assert len(j) == (128 * (mk - 1) + 256 if mk else 0) and score.stoi_num_frames(len(j)) == max(mk - 1, 0)


def test_reference_on_hand_checkable_pairs():
    e, t = S.clip(7001, 3)
    ref, bar, _ = S.stoi_bar(t, t)
    assert (ref["n"], ref["frames"], ref["frames_kept"], ref["segments"]) == (7001, 53, 53, 23)
    assert abs(ref["stoi"] - 1.0) <= bar["stoi"] and abs(ref["estoi"] - 1.0) <= bar["estoi"]
    r3 = score.stoi_reference((3.0 * t.astype(np.float64)).astype(np.float32), t)
    assert abs(r3["stoi"] - 1.0) <= bar["stoi"] and abs(r3["estoi"] - 1.0) <= bar["estoi"]
    # STOI sees magnitudes of the transform only: a sign flip of the estimate changes no band value, so e = -t scores as
    # e = t does -- bit for bit, since every product and sum of the definition commutes with the sign
    rn = score.stoi_reference(-t, t, per_segment=True)
    assert rn["stoi"] == ref["stoi"] and rn["estoi"] == ref["estoi"] and np.array_equal(rn["per_segment"], ref["per_segment"])
    # a negative figure needs opposite ENVELOPES: the target loud where the estimate is quiet
    eo, to = S.opposed_clip()
    ro = score.stoi_reference(eo, to)
    assert ro["stoi"] < -0.5 and ro["segments"] == 31
    # an ordinary pair lies in between, the prefix rule, and too short a clip
    r = score.stoi_reference(e, t)
    assert 0.5 < r["stoi"] < 0.95 and 0.5 < r["estoi"] < 0.95
    assert score.stoi_reference(np.concatenate([e, e]), t) == r
    short = score.stoi_reference(e[:4096], t[:4096])
    assert (short["frames"], short["frames_kept"], short["segments"]) == (30, 30, 0) and math.isnan(short["stoi"]) and math.isnan(short["estoi"])
    zero = score.stoi_reference(e, np.zeros_like(t))
    assert (zero["frames"], zero["frames_kept"], zero["segments"]) == (53, 0, 0) and math.isnan(zero["stoi"])
    imp = score.improvement({"stoi": 0.5, "estoi": 0.25, "snr_db": 1.0}, {"stoi": 0.75, "estoi": 0.75, "snr_db": 2.0})
    assert imp == {"snr_i": 1.0, "stoi_i": 0.25, "estoi_i": 0.5}
    assert "stoi_i" not in score.improvement({"stoi": 0.5, "estoi": 0.25, "snr_db": 1.0}, {"snr_db": 2.0})
    assert len(score.FIELDS) == 12 and len(score.ROW_FIELDS) == 3 and len(score.FIGURES) == 5


def test_the_conditions_hold_on_every_test_clip():
    """The silent-frame margin and the cap on the bar (stoi_checks.conditions, asserted inside stoi_bar) for every clip the
    device is held to, and the compaction clips do what their names say."""
    for e, t in S.length_clips() + [S.clipped_clip(), S.opposed_clip()]:
        S.stoi_bar(e, t)
    kept = {}
    for kind in S.COMPACTION:
        e, t = S.compaction_clip(kind)
        ref, _, _ = S.stoi_bar(e, t)
        kept[kind] = (ref["frames"], ref["frames_kept"], ref["segments"])
    assert kept == {"none": (61, 61, 31), "first": (61, 60, 30), "last": (61, 60, 30), "every_second": (65, 32, 2),
                    "run_leaves_31": (61, 31, 1), "run_leaves_30": (61, 30, 0)}
    # the fixture's signals at 10 kHz through scipy's converter: margins 0.10 and 0.22
    from scipy.signal import resample_poly
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    for ex, lo in (("example2", 0.1), ("example3", 0.2)):
        t10 = resample_poly(g[ex + "_target"].astype(np.float64), 5, 8).astype(np.float32)
        assert S.margin(t10) > lo
        S.stoi_bar(resample_poly(g[ex + "_denoised"].astype(np.float64), 5, 8).astype(np.float32), t10)


# ------------------------------------------------------------------------------ command line
def test_cli_refuses_stoi_without_a_target(tmp_path, capsys):
    from scipy.io import wavfile
    wavfile.write(str(tmp_path / "a.wav"), 16000, np.zeros(800, np.int16))
    one = str(tmp_path / "a.wav")
    try:
        with pytest.raises(SystemExit):
            apply._parse(["--input", one, "--stoi"], "nhans_denoiser")
        assert "--stoi needs --score_against" in capsys.readouterr().err
        a = apply._parse(["--input", one, "--score_against", one, "--stoi"], "nhans_denoiser")
        assert a.stoi is True and apply._parse(["--input", one, "--score_against", one], "nhans_denoiser").stoi is False
    finally:
        apply.FLAGS.score_against, apply.FLAGS.stoi = None, False
        apply.FLAGS.input = apply.Flags.input


# ------------------------------------------------------------------------------ the bar sees planted faults
def test_the_bar_passes_the_reference_and_sees_planted_faults():
    e, t = S.clipped_clip()
    ref = score.stoi_reference(e, t, per_segment=True)
    assert max(S.stoi_ratios(ref, e, t).values()) == 0.0
    # the same definition with numpy's own sums and a transform of twice the length read at every second bin: inside the bar
    _, _, ax, ay, X, Y = S._steps(e, t)
    other = []
    for a in (ax, ay):
        Z = np.fft.fft(a, n=1024, axis=1)[:, 0:512:2]
        p = Z.real ** 2 + Z.imag ** 2
        other.append(np.stack([np.sqrt(p[:, lo:hi].sum(axis=1)) for lo, hi in score.STOI_BANDS], axis=1))
    got = dict(ref, **S._figures(other[0], other[1]))
    r = S.stoi_ratios({k: got[k] for k in score.STOI_FIELDS}, e, t)
    assert 0.0 < max(r.values()) < 0.5, r
    WIDE = 1e6
    ec, tc = S.compaction_clip("run_leaves_31")
    for fault, (a, b), figures in ((S.fault_last_kept_frame_dropped, (e, t), ("stoi", "estoi")),
                                   (S.fault_mask_from_estimate, (ec, tc), ("stoi", "estoi")),
                                   (S.fault_window_once, (e, t), ("stoi", "estoi")),
                                   (S.fault_band_edge_off_by_one, (e, t), ("stoi", "estoi")),
                                   (S.fault_clip_factor, (e, t), ("stoi",)),
                                   (S.fault_columns_before_rows, (e, t), ("estoi",))):
        r = S.stoi_ratios(fault(a, b), a, b, counts=False)
        assert min(r[k] for k in figures) > WIDE, (fault.__name__, r)
