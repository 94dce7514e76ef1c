"""The CPU half of the MVDR tests: the header, the signature table and the exports agree on the new names; the float64
definition (nhans_amd.mvdr) has the properties an MVDR filter has; the simulated scenes of tests/mvdr_checks.py meet the
condition the stage is built for; and the bars of the device tests catch the faults planted in copies of the definition.
Every test prints its figures (pytest -s)."""
import os
import re

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import hip, mvdr

import mvdr_checks as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nhans_mvdr_spectra", "nhans_mvdr_weights", "nhans_mvdr_apply", "nhans_mvdr"]


def test_header_signatures_and_exports_agree():
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = re.findall(r"\bint\s+(nhans_mvdr[a-z_]*)\s*\(([^()]*)\)\s*;", code)
    assert [n for n, _ in decls] == NAMES
    order = list(hip.SIGNATURES)
    assert [n for n in order if n.startswith("nhans_mvdr")] == NAMES
    assert order.index("nhans_mvdr") + 1 == order.index("nhans_profile_json")       # declared before nhans_profile_json
    for name, params in decls:
        assert len(params.split(",")) == len(hip.SIGNATURES[name][1]), name
        assert name in hip.EXPORTS
    for macro, value in (("NHANS_MVDR_MAX_CHANNELS", hip.MVDR_MAX_CHANNELS), ("NHANS_MVDR_FIELDS", hip.MVDR_FIELDS),
                         ("NHANS_MVDR_LOGGAIN", hip.MVDR_LOGGAIN)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert hip.MVDR_FIELDS == len(mvdr.FIELDS) and hip.MVDR_MAX_CHANNELS == mvdr.MAX_CHANNELS
    assert re.search(r"#define NHANS_ABI_VERSION (\d+)", header).group(1) == "5" == str(hip.ABI_VERSION)
    kernels = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    assert "kMvdrMaxChannels = %d, kMvdrFields = %d, kMvdrLogGain = %d" % (mvdr.MAX_CHANNELS, len(mvdr.FIELDS), hip.MVDR_LOGGAIN) in kernels
    assert "kMvdrRun = %d" % hip.MVDR_RUN in kernels


def _hermitian_pd(rng, K, C):
    a = rng.standard_normal((K, C, C + 2)) + 1j * rng.standard_normal((K, C, C + 2))
    return a @ np.conj(a.transpose(0, 2, 1))


@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_distortionless_for_a_rank_one_speech_covariance(C):
    """Phi_s = d d^H: w^H d = 1 at the reference channel's scale, d_ref = 1."""
    rng = np.random.default_rng(100 + C)
    K = mvdr.BINS
    d = rng.standard_normal((K, C)) + 1j * rng.standard_normal((K, C))
    for ref in (0, C - 1):
        dr = d / d[:, ref:ref + 1]
        ps = 3.7 * dr[:, :, None] * np.conj(dr[:, None, :])
        pn = _hermitian_pd(rng, K, C)
        w, fb = mvdr.weights(ps, pn, ref, 0.0)
        got = np.einsum("kc,kc->k", np.conj(w), dr)
        cond = np.linalg.cond(pn).max()
        print("C %d ref %d: max |w^H d - 1| = %.3e (largest cond %.3e)" % (C, ref, np.abs(got - 1).max(), cond))
        assert not fb.any()
        assert np.abs(got - 1).max() <= 64 * C * C * M.U * cond


def test_unchanged_by_scaling_either_covariance():
    rng = np.random.default_rng(7)
    ps, pn = _hermitian_pd(rng, 50, 4), _hermitian_pd(rng, 50, 4)
    w0, _ = mvdr.weights(ps, pn, 1, mvdr.LOADING)
    for a, b in ((8.0, 1.0), (1.0, 0.25), (2.0 ** 20, 2.0 ** -30)):        # powers of four (the root is exact): the same bits
        w, fb = mvdr.weights(a * ps, b * pn, 1, mvdr.LOADING)
        assert not fb.any() and np.array_equal(w, w0), (a, b)
    w, _ = mvdr.weights(3.3 * ps, 0.7 * pn, 1, mvdr.LOADING)
    assert np.abs(w - w0).max() <= 1e-12 * np.abs(w0).max()


def test_commutes_with_a_permutation_of_the_channels():
    x = M.random_clip(12, 4, 31)
    m = M.random_mask(12, 32)
    perm = [2, 0, 3, 1]
    a = mvdr.reference(x, m, ref=2)
    b = mvdr.reference(x[:, perm], m, ref=perm.index(2))
    print("permuted: max |y - y'| = %.3e of %.3e" % (np.abs(a["y"] - b["y"]).max(), np.abs(a["y"]).max()))
    assert np.abs(a["w"][:, perm] - b["w"]).max() <= 1e-9 * np.abs(a["w"]).max()
    assert np.abs(a["y"] - b["y"]).max() <= 1e-9 * np.abs(a["y"]).max()


@pytest.mark.parametrize("value", [1.0, 0.0])
def test_a_mask_of_all_ones_or_zeros_returns_the_reference_channel(value):
    x = M.random_clip(9, 3, 41)
    for ref in (0, 2):
        r = mvdr.reference(x, np.full((9, mvdr.BINS), value, np.float32), ref=ref)
        assert r["record"]["fallback_bins"] == mvdr.BINS and r["fallback"].all()
        assert np.array_equal(r["y"], r["X"][ref])
        assert r["record"]["energy_out"] == r["record"]["energy_ref"]


def test_mask_values():
    v = np.array([[-1.0, 0.0, 0.25, 1.0, 7.0, np.nan, np.inf, -np.inf]])
    assert np.array_equal(mvdr.mask_values(v), [[0, 0, 0.25, 1, 1, 0, 1, 0]])
    g = np.array([[-np.inf, -1.0, 0.0, 3.0, np.inf, np.nan]])
    assert np.allclose(mvdr.mask_values(g, loggain=True), [[0, np.exp(-1.0), 1, 1, 1, 0]], rtol=1e-15)
    for bad in (dict(channels=0, ref=0, loading=0.0), dict(channels=9, ref=0, loading=0.0), dict(channels=2, ref=2, loading=0.0),
                dict(channels=2, ref=-1, loading=0.0), dict(channels=2, ref=0, loading=1.5), dict(channels=2, ref=0, loading=-1e-9)):
        with pytest.raises(ValueError):
            mvdr.check(**bad)


_scores = {}


def scores(name, C):
    if (name, C) not in _scores:
        sc = M.scene(name, C)
        _scores[(name, C)] = (M.scene_scores(sc, sc["trained_mask"]), M.scene_scores(sc, sc["oracle_mask"]))
    return _scores[(name, C)]


@pytest.mark.parametrize("name", M.SCENES)
@pytest.mark.parametrize("C", [2, 4])
def test_the_scenes_meet_the_condition(name, C):
    """With the trained mask the MVDR output beats the better of channel 0 and the channel mean by >= 3 dB; with the oracle
    mask it beats the trained mask on channel 0 by >= 3 dB.  Float64, the library's transform pair, interior samples.
    Measured: 12.3 / 8.8 dB (example2, C = 2), 8.3 / 6.4 (C = 4), 14.2 / 12.0 (example3, C = 2), 9.4 / 10.5 (C = 4)."""
    tr, orc = scores(name, C)
    print("%s C %d: channel 0 %.2f, mean %.2f, mask alone %.2f, MVDR trained %.2f, MVDR oracle %.2f dB; fallback bins %d, %d" % (
        name, C, tr["ref"], tr["mean"], tr["mask"], tr["mvdr"], orc["mvdr"], tr["fallback_bins"], orc["fallback_bins"]))
    assert tr["fallback_bins"] == 0 and orc["fallback_bins"] == 0
    assert tr["mvdr"] - max(tr["ref"], tr["mean"]) >= M.MARGIN_DB
    assert orc["mvdr"] - tr["mask"] >= M.MARGIN_DB


def test_the_bars_pass_the_definition_and_catch_the_planted_faults():
    x, m = M.random_clip(20, 3, 51), M.random_mask(20, 52)
    X32 = mvdr.spectra(x).astype(np.complex64)
    r = mvdr.reference(x, m, ref=1, X=X32)
    y32 = r["y"].astype(np.complex64)
    lm32 = np.log(np.maximum(np.abs(y32.astype(np.complex128)), mvdr.FLOOR)).astype(np.float32)
    ph32 = np.angle(y32.astype(np.complex128)).astype(np.float32)
    mv = mvdr.mask_values(m)
    assert M.check_covariances("definition", r["phi_s"], r["phi_n"], X32, mv).ok
    vw = M.check_weights("definition", r["w"], r["phi_s"], r["phi_n"], 1, mvdr.LOADING)
    assert vw.ok and vw.judged.all(), vw.message
    vf = M.check_filter("definition", y32, lm32, ph32, X32, r["w"])
    assert vf.ok, vf.message
    print("definition through the bars: weights %.3f, filter %.3f, lm %.3f, ph %.3f of the bar" % (vw.rel, vf.rel, vf.rel_lm, vf.rel_ph))
    # w^T x in place of w^H x
    bad = mvdr.apply(X32, np.conj(r["w"])).astype(np.complex64)
    v = M.check_filter("w^T x", bad, lm32, ph32, X32, r["w"])
    assert not v.ok and v.rel > 1e3, v.rel
    # the two masks swapped
    v = M.check_covariances("swapped", r["phi_n"], r["phi_s"], X32, mv)
    assert not v.ok and v.rel > 1e3
    ws, _ = mvdr.weights(r["phi_n"], r["phi_s"], 1, mvdr.LOADING)
    v = M.check_weights("swapped", ws, r["phi_s"], r["phi_n"], 1, mvdr.LOADING)
    assert not v.ok and v.rel > 1e3
    # a rows fault: the analysis rows' + 1e-5 in place of the max
    v = M.check_filter("+1e-5", y32, np.log(np.abs(y32.astype(np.complex128)) + 1e-5).astype(np.float32), ph32, X32, r["w"])
    assert not v.ok


def test_the_loading_left_out_at_one_frame_is_caught():
    """T = 1: Phi_n has rank one, and only the loading makes it positive definite.  With it no bin falls back and every
    bin is well enough conditioned to be judged; without it the second pivot is zero or rounding."""
    x, m = M.random_clip(1, 3, 61), np.full((1, mvdr.BINS), 0.5, np.float32)
    X32 = mvdr.spectra(x).astype(np.complex64)
    r = mvdr.reference(x, m, X=X32)
    assert r["record"]["fallback_bins"] == 0
    v = M.check_weights("T = 1", r["w"], r["phi_s"], r["phi_n"], 0, mvdr.LOADING)
    assert v.ok and v.judged.all(), v.message
    w0, fb0 = mvdr.weights(r["phi_s"], r["phi_n"], 0, 0.0)
    v = M.check_weights("no loading", w0, r["phi_s"], r["phi_n"], 0, mvdr.LOADING)
    print("T = 1 without the loading: %d bins fall back; %s" % (int(fb0.sum()), v.message))
    assert not v.ok


def test_scene_fault_costs_decibels():
    """The planted faults on a scene: each loses far more than the 0.05 dB the device is held to."""
    sc = M.scene("example2", 2)
    good = scores("example2", 2)[0]["mvdr"]
    for name, fn in (("w^T x", M.reference_transposed), ("masks swapped", M.reference_masks_swapped)):
        got = M.scene_scores(sc, sc["trained_mask"], reference=fn)["mvdr"]
        print("%s: %.2f dB for %.2f" % (name, got, good))
        assert good - got > 3.0


# ---- the command line: --array mvdr [--array_ref R] [--array_post none|mask|net] ------------------------------------
def _wav(path, channels, n=8000):
    from scipy.io import wavfile
    rng = np.random.default_rng(channels)
    x = (3000 * rng.standard_normal((n, channels) if channels > 1 else n)).astype(np.int16)
    wavfile.write(str(path), 16000, x)
    return x


def test_array_flags_and_their_argument_errors(tmp_path, capsys):
    from nhans_amd import apply
    stereo, mono, nine = tmp_path / "stereo.wav", tmp_path / "mono.wav", tmp_path / "nine.wav"
    _wav(stereo, 2), _wav(mono, 1), _wav(nine, 9)
    keep = dict(vars(apply.FLAGS))
    try:
        a = apply._parse(["--input", str(stereo), "--array", "mvdr", "--array_ref", "1", "--array_post", "net"], "nhans")
        assert (a.array, a.array_ref, a.array_post) == ("mvdr", 1, "net")
        a = apply._parse(["--input", str(stereo)], "nhans")
        assert (a.array, a.array_ref, a.array_post) == (None, 0, "none")
        d = tmp_path / "dir"
        d.mkdir()
        _wav(d / "a.wav", 2), _wav(d / "b.wav", 1)
        bad = [(["--input", str(mono), "--array", "mvdr"], "is mono"),
               (["--input", str(d), "--array", "mvdr"], "b.wav is mono"),
               (["--input", str(nine), "--array", "mvdr"], "up to 8 channels"),
               (["--input", str(stereo), "--array", "mvdr", "--array_ref", "2"], "--array_ref must be in 0 ... 1"),
               (["--input", str(stereo), "--array", "mvdr", "--array_ref", "-1"], "--array_ref must be in 0 ... 1"),
               (["--input", str(stereo), "--array", "gev"], "invalid choice"),
               (["--input", str(stereo), "--array", "mvdr", "--array_post", "twice"], "invalid choice"),
               (["--input", str(stereo), "--array_ref", "1"], "need --array mvdr"),
               (["--input", str(stereo), "--array_post", "mask"], "need --array mvdr"),
               (["--input", str(stereo), "--array", "mvdr", "--online_ms", "100"], "does not go with --online_ms"),
               (["--input", str(stereo), "--array", "mvdr", "--convert_on", "gpu"], "does not go with --convert_on gpu"),
               (["--input", str(stereo), "--array", "mvdr", "--fbank_out", str(tmp_path / "f.npy")], "does not go with --fbank_out")]
        for argv, text in bad:
            with pytest.raises(SystemExit) as e:
                apply._parse(argv, "nhans")
            assert e.value.code == 2, argv
            assert text in capsys.readouterr().err, argv
    finally:
        for k, v in keep.items():
            setattr(apply.FLAGS, k, v)
        for k in set(vars(apply.FLAGS)) - set(keep):
            delattr(apply.FLAGS, k)


def test_array_reader_keeps_the_channels_on_today_s_scale(tmp_path):
    """The mean of what --array hands over is the signal the file gives today, to float32 rounding of each channel."""
    from nhans_amd import apply
    x = _wav(tmp_path / "s.wav", 3, 400 + 160 * 20 + 77)
    ca, cb, mixed = apply.handle_array_signals(str(tmp_path / "s.wav"), None, None)
    today = apply.trim_to_frames(apply.normalise(apply.read_wav(str(tmp_path / "s.wav"))))
    assert mixed.shape == (len(today), 3) and mixed.dtype == np.float32
    assert np.abs(mixed.astype(np.float64).mean(axis=1) - today).max() <= 2.0 ** -23 * np.abs(mixed).max()
    assert len(ca) == len(cb) and not ca.any()
    assert apply.handle_array_signals(str(tmp_path / "missing.wav"), None, None) is None
