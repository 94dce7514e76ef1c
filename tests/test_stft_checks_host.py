"""CPU half of the STFT / inverse STFT domain tests (tests/stft_checks.py): the classes are what they claim to be, the
float32 yardstick alone stays inside the caps on every class, and the comparison catches the faults it is for and names
their place."""
import numpy as np
import pytest

import stft_checks as C
import oracle.nhans_oracle as O


@pytest.fixture(scope="module")
def classes():
    return C.analysis_classes()


@pytest.fixture(scope="module")
def inv_classes(classes):
    return C.inverse_classes(C.cpu32_features(classes[0][1])[1])


def test_analysis_classes_are_what_they_claim(classes):
    assert len(classes) == 11
    for name, w in classes:
        assert w.dtype == np.float32 and w.shape == (C.SAMPLES,), name
        assert O.stft(w).shape == (C.FRAMES, C.BINS), name
    by = {name.split()[0]: w for name, w in classes}
    assert np.abs(by["2"]).max() > 20000 and np.array_equal(by["2"], np.rint(by["2"]))        # int16 scale, not normalised
    fade = by["9"]
    assert np.abs(fade[:100]).max() > 1.0 and np.abs(fade[-40:]).max() < 1e-43 and (fade[-400:] == 0).any()      # underflows to 0
    sub = (np.abs(fade) > 0) & (np.abs(fade) < 1.17549435e-38)
    assert sub.sum() > 300                                                                     # the whole denormal range
    # the suspect of the fade: frames that hold bins whose larger component is non-zero and below the smallest normal
    X = O.stft(fade)
    big = np.maximum(np.abs(X.real), np.abs(X.imag))
    assert int(((big > 0) & (big < 1.17549435e-38)).any(axis=1).sum()) == 3
    # exact-bin cosines: everything off bins k - 1 .. k + 1 is the float32 rounding of the samples
    mag = np.abs(O.stft(by["6"]))
    near = np.zeros(C.BINS, bool)
    for k in (1, 37, 100, 199):
        near[k - 1:k + 2] = True
        assert mag[:, k].min() > 99.0
    assert mag[:, ~near].max() < 1e-5
    assert all(b in C.MIRRORED for b in (37, 199)) and all(b not in C.MIRRORED for b in (1, 100, 200, 0))
    mag = np.abs(O.stft(by["7"]))
    assert mag[:, 200].min() > 199.0 and mag[:, :199].max() < 1e-10
    assert not by["11"].any()


def test_frame_count_clips_cover_every_tail_and_run_boundary():
    tails = C.count_tails()
    assert 0 in tails and 159 in tails and len(set(tails)) > 40
    clips = C.count_clips()
    assert [1 + (len(w) - C.WIN) // C.HOP for w in clips] == list(range(1, 51))
    assert [(len(w) - C.WIN) % C.HOP for w in clips] == tails
    assert sum(range(1, 51)) < 2000
    # clips that end exactly on, one short of and one past a run of either kernel
    for run in (C.STFT_RUN, C.ISTFT_RUN):
        assert {run - 1, run, run + 1, 2 * run, 2 * run + 1} <= set(range(1, 51))


def test_float32_yardstick_stays_inside_the_analysis_cap_on_every_class(classes):
    for name, w in classes:
        r = C.yardstick_ratio(name, [w])
        lm, ph = C.cpu32_features(w)
        v = C.check_analysis(name, 0, lm, ph, w, r)
        print("analysis %-36s ratio %.3e  K x ratio / cap %.3f" % (name, r, C.K * r / C.CAP_ANALYSIS))
        assert C.K * r < C.CAP_ANALYSIS, name
        assert v.ok, v.message                      # finite, in range, floor, phase: the restatement meets all of them
        assert v.rel == r
    zl, zp = C.cpu32_features(classes[10][1])
    assert np.abs(zl - C.FLOOR).max() < C.FLOOR_TOL          # (angle(-0 + 0j) = pi on the CPU: the phase of a zero bin is free)
    r = C.yardstick_ratio("count", C.count_clips())
    assert C.K * r < C.CAP_ANALYSIS


def test_float32_yardstick_stays_inside_the_inverse_cap_on_every_class(inv_classes):
    assert len(inv_classes) == 9
    cases = [(n, lm, ph) for n, lm, ph in inv_classes] + [("count T=%d" % len(lm), lm, ph) for lm, ph in C.count_spectra()]
    for name, lm, ph in cases:
        assert lm.dtype == np.float32 and ph.dtype == np.float32
        v = C.check_inverse(name, 0, C.cpu32_inverse(lm, ph), lm, ph, f_share=C.F_INVERSE)
        if not name.startswith("count"):
            print("inverse %-36s err_cpu32 / max %.3e  bar / cap %.3f" % (name, v.err_cpu32 / v.m, v.bar / (C.CAP_INVERSE * v.m)))
        assert v.ok, v.message
        assert C.K * v.err_cpu32 + C.F_INVERSE * v.m < C.CAP_INVERSE * v.m, name
    by = {n.split()[0]: (lm, ph) for n, lm, ph in inv_classes}
    for k in ("7a", "7b"):              # the slack the ABI grants phases outside [-pi, pi] leaves the bar far below the cap
        v = C.check_inverse(k, 0, C.cpu32_inverse(*by[k]), *by[k], phase_slack=C.PHASE_SLACK_7PI)
        slack = C.PHASE_SLACK_7PI * C.phase_sensitivity(by[k][0])
        assert v.ok and 0 < slack < 4e-6 * v.m and abs(v.bar - (C.K * v.err_cpu32 + slack)) < 1e-18, (slack, v.m)
    assert by["2"][0].max() <= C.FLOOR and by["3"][0].max() > 15.9
    assert (by["4a"][0][0::2] == 6.0).all() and (by["4b"][0][1::2] == 6.0).all() and (by["4a"][0][1::2] < -11).all()
    assert set(np.unique(by["5"][1])) == {np.float32(-np.pi), np.float32(0), np.float32(np.pi)}
    assert np.abs(by["7a"][1]).min() > 5 * np.pi and by["7a"][1].min() > 0 > by["7b"][1].max()


# ---- sensitivity: each fault planted in the float32 restatement fails the comparison at the right place ---------------
def _analysis_fault(classes, cls, fault):
    name, w = classes[cls]
    r = C.yardstick_ratio(name, [w])
    good = C.check_analysis(name, 0, *C.cpu32_features(w), w, r)
    assert good.ok, good.message
    v = C.check_analysis(name, 0, *C.cpu32_features(w, fault), w, r)
    assert not v.ok
    return v


def test_comparison_catches_swapped_mirror_bins(classes):
    v = _analysis_fault(classes, 5, "mirror_swap")                    # exact-bin cosines: bin 37 is a mirrored bin
    assert v.worst[1] in (37, 57), v.message
    assert "class 6 exact-bin" in v.message and ("bin 37" in v.message or "bin 57" in v.message)


def test_comparison_catches_a_dropped_conjugate(classes):
    for cls in (0, 7):                                                # noise; the off-bin cosine, whose peak is mirrored
        v = _analysis_fault(classes, cls, "conj_dropped")
        assert v.worst[1] in C.MIRRORED, v.message
        assert "bin %d" % v.worst[1] in v.message and "phase off" in v.message
    assert _analysis_fault(classes, 7, "conj_dropped").worst[1] in (37, 38)


def test_comparison_catches_a_leak_between_frames_that_a_per_clip_bar_hides(classes):
    name, w = classes[9]
    v = _analysis_fault(classes, 9, "leak")
    assert v.worst[0] == C.LEAK_FROM + 1, v.message
    assert "frame %d" % (C.LEAK_FROM + 1) in v.message and "class 10" in v.message
    assert int((v.err > v.bar).sum()) == 1
    # the per-clip bar of the older tests does not see it
    X = O.stft(w)
    assert np.abs(C.linear(*C.cpu32_features(w, "leak")) - X).max() <= 1e-5 * np.abs(X).max()


def test_comparison_catches_a_zeroed_last_frame_of_a_run():
    w = C.count_clips()[29]                                           # 30 frames, 7 * 137 % 160 untrimmed samples... of noise
    r = C.yardstick_ratio("count", C.count_clips())
    v = C.check_analysis("count", 29, *C.cpu32_features(w, "run_end_zeroed"), w, r)
    assert not v.ok and v.worst[0] == C.STFT_RUN - 1, v.message
    assert "clip 29, frame 22" in v.message
    assert int((v.err > v.bar).sum()) == 1


def test_comparison_catches_a_kept_nyquist_imaginary_part(inv_classes):
    by = {n.split()[0]: (n, lm, ph) for n, lm, ph in inv_classes}
    name, lm, ph = by["6"]
    assert C.check_inverse(name, 0, C.cpu32_inverse(lm, ph), lm, ph, f_share=0.0).ok
    v = C.check_inverse(name, 3, C.cpu32_inverse(lm, ph, "nyquist_imag"), lm, ph, f_share=2e-6)
    assert not v.ok and "class 6 phase at bins 0 and 200, clip 3" in v.message and "at sample" in v.message
    # phases of a real signal's Nyquist bin are 0 or pi: the same fault is invisible on class 1, which is why class 6 exists
    name, lm, ph = by["1"]
    assert C.check_inverse(name, 0, C.cpu32_inverse(lm, ph, "nyquist_imag"), lm, ph, f_share=2e-6).ok
