"""Online enhancement on the host: the output-count formula against a brute-force simulation of sample finality, the
fixed-peak normalisation against apply.normalise, and the command-line flag."""
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, online, spec


def _final_samples(n, ended):
    """Brute force: output sample s is final when every frame that covers it has been synthesised with offline bits --
    the frame's window is complete (17 frames of look-ahead exist, or the stream has ended) and so is its iSTFT pair
    partner (2k, 2k+1) -- and no frame that could still arrive covers it; after the end, the offline length."""
    T = online.num_frames(n)
    if ended:
        return 0 if T == 0 else (T - 1) * spec.HOP + spec.WIN
    def synth_ok(f):
        ready = lambda g: g + online.LOOKAHEAD < T
        return ready(f) and ready(f ^ 1)
    s = 0
    while True:
        covering = [f for f in range(max(0, (s - spec.WIN) // spec.HOP), s // spec.HOP + 1)
                    if f * spec.HOP <= s < f * spec.HOP + spec.WIN]
        if not all(synth_ok(f) for f in covering):
            return s
        s += 1


def test_out_counts_formula_matches_a_brute_force_finality_simulation():
    for n in list(range(0, 400 * 20, 53)) + [399, 400, 559, 560, 400 + 160 * 17, 400 + 160 * 18, 400 + 160 * 19 - 1]:
        for ended in (False, True):
            assert online.emitted(n, ended) == _final_samples(n, ended), (n, ended)


def test_out_counts_of_a_push():
    assert online.out_counts([0], [400 + 160 * 18], [False]) == [320]
    assert online.out_counts([0], [400 + 160 * 18 + 10], [True]) == [400 + 160 * 18]
    assert online.out_counts([0, 100], [399, 0], [True, False]) == [0, 0]
    assert online.out_counts([5000], [0], [False], [True]) == [0]
    assert online.latency_ms() == (185.0, 205.0)


def test_normalise_fixed_is_apply_normalise_at_the_whole_file_peak():
    rng = np.random.default_rng(1)
    x16 = (rng.standard_normal(20000) * 3000).astype(np.int16)
    for x in (x16, rng.standard_normal(5000).astype(np.float32)):
        peak = np.max(np.abs(x))
        a, b = online.normalise_fixed(x, peak), apply.normalise(x)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()


def test_online_ms_flag_parses_and_refuses_a_directory(tmp_path):
    a = apply._parse(["--input", "x.wav", "--online_ms", "20"], "nhans_denoiser")
    assert a.online_ms == 20.0
    with pytest.raises(SystemExit):
        apply._parse(["--input", str(tmp_path), "--online_ms", "20"], "nhans_denoiser")
    with pytest.raises(SystemExit):
        apply._parse(["--input", "x.wav", "--online_ms", "0"], "nhans_separator")
    apply._parse(["--input", "x.wav"], "nhans_denoiser")
    assert apply.FLAGS.online_ms is None
