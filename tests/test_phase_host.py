"""The CPU half of the phase-refinement tests: the float64 definition (nhans_amd.phase) against the oracle's transforms, the
float32 restatement's yardstick on every class, the planted faults, and the host-only contract of the binding (no GPU)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import nhans_amd  # noqa: F401
from nhans_amd import hip, phase
import oracle.nhans_oracle as O

import phase_checks as P

CLASSES = P.classes()


@pytest.mark.parametrize("name,lm,t", CLASSES, ids=[c[0] for c in CLASSES])
def test_project_reference_is_the_oracles_round_trip(name, lm, t):
    z = t.astype(np.complex128)
    want = O.stft(O.recover_samples(lm.astype(np.float64), np.angle(phase.unit(z))))
    got = phase.project_reference(lm, z)
    assert got.shape == want.shape == lm.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_windows_are_the_oracles():
    assert np.array_equal(phase.analysis_window(), O.hann_periodic())
    assert np.array_equal(phase.synthesis_window(), O.istft_window())


def test_unit_convention():
    z = np.array([0.0, 1e-40, 1e-39 - 1e-39j, 3e-30 + 4e-30j, -2.0j, 1.1754944e-38], dtype=np.complex128)
    u = phase.unit(z)
    assert np.array_equal(u[:3], [1.0, 1.0, 1.0])
    assert np.allclose(u[3:], [0.6 + 0.8j, -1.0j, 1.0], atol=1e-15)


def test_reference_with_no_iteration_returns_its_input():
    lm, ph = P.uniform_case(7, 11)
    r = phase.reference(lm, ph, 0)
    assert r["phase"] is ph or np.array_equal(r["phase"].view(np.uint32), ph.view(np.uint32))
    assert r["phase"].dtype == np.float32 and len(r["inc"]) == 0
    assert np.abs(r["wave"] - O.recover_samples(lm.astype(np.float64), ph.astype(np.float64))).max() < 1e-12
    for bad in (dict(iters=-1), dict(iters=257), dict(iters=1, alpha=1.0), dict(iters=1, alpha=-0.1)):
        with pytest.raises(ValueError):
            phase.reference(lm, ph, **bad)


def test_reference_iteration_is_the_definition():
    lm, ph = P.uniform_case(9, 12)
    r = phase.reference(lm, ph, 3, alpha=0.5, states=True)
    t0 = np.exp(1j * ph.astype(np.float64))
    d0 = phase.project_reference(lm, t0)
    d1 = phase.project_reference(lm, d0)                   # d_{-1} := d_0: t_1 = d_0
    t2 = d1 + 0.5 * (d1 - d0)
    d2 = phase.project_reference(lm, t2)
    t3 = d2 + 0.5 * (d2 - d1)
    assert np.array_equal(r["t"][1], d0) and np.array_equal(r["t"][2], t2) and np.array_equal(r["t"][3], t3)
    assert np.array_equal(r["phase"], np.angle(t3))
    a = np.exp(lm.astype(np.float64))
    assert r["inc"][2] == ((np.abs(d2) - a) ** 2).sum() / (a ** 2).sum()


def test_inconsistency_falls_on_the_demo_magnitudes():
    """The figures of the feature's case: from -19.8 dB (the mixture's phase, inc[0]) to -27.9 dB after 8 plain iterations
    (inc[8], the projection of t_8) on example2."""
    lm, ph, _, _ = P.demo_rows("example2")
    inc = phase.reference(lm, ph, 9)["inc"]
    db = 10 * np.log10(inc)             # inc is a ratio of squares: 10 log10 of it is 20 log10 of the ratio of norms
    assert abs(db[0] - -19.8) < 0.05 and abs(db[8] - -27.9) < 0.05, db


@pytest.mark.parametrize("name,lm,t", CLASSES, ids=[c[0] for c in CLASSES])
def test_restatement_sits_under_the_cap(name, lm, t):
    ratio = P.yardstick_ratio(name, lm, t)
    print("%s: ratio %.3e" % (name, ratio))
    assert 0.0 < ratio and P.K * ratio < P.CAP / 5.0
    v = P.check_project(name, P.cpu32_project(lm, t), lm, t, ratio)
    assert v.ok, v.message


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_faults_are_caught_and_located(fault):
    name, lm, t = next(c for c in CLASSES if c[0] == "uniform T=%d" % (2 * P.RUN + 1))
    ratio = P.yardstick_ratio(name, lm, t)
    v = P.check_project(name, P.cpu32_project(lm, t, fault=fault), lm, t, ratio)
    assert not v.ok and "above the bar" in v.message, fault
    f, k = v.worst
    if fault == "halo_dropped":
        assert f in (P.RUN - 2, P.RUN - 1, P.RUN), v.message        # the frames that hold the 80 samples without frame RUN - 2
    elif fault == "conj_dropped":
        assert k in P.MIRRORED, v.message
    else:
        assert "frame %d of" % f in v.message and "bin %d" % k in v.message


def test_a_quiet_frame_is_judged_by_its_neighbours_scale():
    name, lm, t = next(c for c in CLASSES if c[0].startswith("loud and quiet"))
    sc = P.scale(lm)
    assert np.all(sc == 1.0)            # every quiet frame has a loud one within two frames
    assert P.scale(np.log(np.array([[1.0], [1e-4], [1e-4], [1e-4], [1e-4], [1e-4]])))[3] == pytest.approx(1e-4)


def test_run_length_and_binding_constants_match_the_kernel():
    text = open(os.path.join(ROOT, "n-hans_amd", "csrc", "nhans_kernels.h")).read()
    assert int(re.search(r"constexpr int kPhaseRun = (\d+);", text).group(1)) == P.RUN == hip.PHASE_RUN == phase.RUN
    assert int(re.search(r"constexpr int kPhaseMaxIters = (\d+);", text).group(1)) == hip.PHASE_MAX_ITERS == phase.MAX_ITERS
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    assert "#define NHANS_PHASE_MAX_ITERS %d" % hip.PHASE_MAX_ITERS in header
    for fn in ("nhans_phase_set_alpha", "nhans_phase_project", "nhans_phase_refine"):
        assert fn in hip.SIGNATURES and re.search(r"\bint %s\(" % fn, header)


def test_free_running_restatement_is_a_yardstick_on_the_uniform_class():
    lm, ph = P.uniform_case(30, 4030)
    for alpha in (0.0, 0.5):
        _, inc_rel, wave_abs, wave_max = P.free_running_yardstick(lm, ph, 8, alpha)
        print("alpha %g: restatement inc_rel %.3e wave %.3e of %.3e" % (alpha, inc_rel, wave_abs, wave_max))
        assert inc_rel < P.ILL and wave_abs < P.ILL * wave_max


def test_command_line_refuses_iterations_out_of_range_and_with_the_online_path(capsys):
    from nhans_amd import apply
    for argv, word in ((["--phase_iters", "4", "--online_ms", "100"], "--online_ms"), (["--phase_iters", "257"], "0 ... 256"),
                       (["--phase_iters", "-1"], "0 ... 256"), (["--phase_iters", "2", "--phase_alpha", "1.0"], "[0, 1)")):
        with pytest.raises(SystemExit):
            apply._parse(["--input", "x.wav"] + argv, "nhans")
        assert word in capsys.readouterr().err
    assert apply.Flags.phase_iters == 0 and apply.Flags.phase_alpha == 0.0 and apply._phase_kw() == {}
