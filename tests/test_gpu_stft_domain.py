"""nhans_stft_features and nhans_istft over the whole input domain of the C ABI, against the float64 oracle at the bar of
tests/stft_checks.py: per FRAME in the analysis direction (a loud frame must not hide a quiet one), per clip in the
inverse; signal classes that walk the preconditions of the hardware transcendentals (denormal bins, the floor, large and
tiny magnitudes, unreduced phases), every frame count 1 .. 50 with untrimmed tails, canaries behind the outputs.
profiles/stft_domain/README.md holds the measured figures.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine, hip
import stft_checks as C

pytestmark = pytest.mark.gpu

CANARY = 12345.678


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def _stft(eng, wavs, max_frames=0, want_phase=True):
    """One ragged nhans_stft_features launch into buffers with one canary row behind the last frame.
    -> (lm [T,201], ph or None, frame offsets)."""
    off = C.offsets([len(w) for w in wavs])
    nfr = [int(eng.lib.nhans_num_frames(len(w))) for w in wavs]
    foff = C.offsets([min(t, max_frames) if max_frames > 0 else t for t in nfr])
    wav_t = torch.from_numpy(np.concatenate(wavs)).cuda()
    lm = torch.full((foff[-1] + 1, C.BINS), CANARY, dtype=torch.float32, device="cuda")
    ph = torch.full_like(lm, CANARY) if want_phase else None
    hip.check(eng.lib.nhans_stft_features(eng.handle, hip.ptr(wav_t), hip.i64_array(off), len(wavs), max_frames,
                                          hip.ptr(lm), hip.ptr(ph), eng._stream()))
    lm = lm.cpu().numpy()
    ph = ph.cpu().numpy() if want_phase else None
    assert (lm[-1] == np.float32(CANARY)).all(), "the row behind the last log-magnitude row was written"
    assert ph is None or (ph[-1] == np.float32(CANARY)).all(), "the row behind the last phase row was written"
    return lm[:-1], (ph[:-1] if want_phase else None), foff


@pytest.fixture(scope="module")
def analysis(eng):
    classes = C.analysis_classes()
    lm, ph, foff = _stft(eng, [w for _, w in classes])
    assert foff == [C.FRAMES * i for i in range(len(classes) + 1)]
    return classes, lm, ph, foff


def test_every_analysis_class_meets_the_per_frame_bar(analysis):
    classes, lm, ph, foff = analysis
    bad = []
    for i, (name, w) in enumerate(classes):
        ratio = C.yardstick_ratio(name, [w])
        v = C.check_analysis(name, i, lm[foff[i]:foff[i + 1]], ph[foff[i]:foff[i + 1]], w, ratio)
        print("analysis %-36s rel_hip %.3e  rel_cpu32 %.3e  hip/cpu32 %6.2f  max err %.3e  worst (frame, bin) %s %s" % (
            name, v.rel, ratio, v.rel / max(ratio, 1e-300) if ratio else float("nan"), float(v.err.max()), v.worst,
            "" if v.ok else "FAIL"))
        if not v.ok:
            bad.append(v.message)
    assert not bad, "\n".join(bad)


def test_engine_entry_point_gives_the_same_bits(eng, analysis):
    classes, lm, ph, foff = analysis
    wavs = [w for _, w in classes]
    lm2, ph2 = eng.stft_features(torch.from_numpy(np.concatenate(wavs)).cuda(), C.offsets([len(w) for w in wavs]))
    assert np.array_equal(lm2.cpu().numpy().view(np.int32), lm.view(np.int32))
    assert np.array_equal(ph2.cpu().numpy().view(np.int32), ph.view(np.int32))


def test_silence_and_bins_below_the_smallest_normal(analysis):
    """Zeros: the floor within 1e-6 and phase exactly 0.  The fade: bins whose components are both below the smallest normal
    float32 (1.18e-38) have no reciprocal on the hardware unit; their phase is that of the axis of the larger component --
    0, +-pi/2 or +-pi --, the limit include/nhans_hip.h states."""
    classes, lm, ph, foff = analysis
    z = slice(foff[10], foff[11])
    print("zeros: max |lm - ln 1e-5| %.3e" % np.abs(lm[z].astype(np.float64) - C.FLOOR).max())
    assert np.abs(lm[z].astype(np.float64) - C.FLOOR).max() < C.FLOOR_TOL
    assert not ph[z].any()
    X = C.O.stft(classes[8][1])
    big = np.maximum(np.abs(X.real), np.abs(X.imag))
    sub = big < 1e-39                        # float32 rounding down there is 1.4e-45 per operation: still below 1.18e-38
    assert (sub & (big > 0)).any(axis=1).sum() >= 3
    p = ph[foff[8]:foff[9]]
    quarter = np.abs(p[sub]) / np.float32(np.pi / 2)
    print("fade: %d bins below 1e-39, %d of them non-finite, phases %s" % (sub.sum(), (~np.isfinite(p[sub])).sum(),
                                                                           np.unique(p[sub])[:8]))
    assert np.isfinite(p[sub]).all()
    assert np.isin(quarter, [0.0, 1.0, 2.0]).all(), np.unique(p[sub])


@pytest.fixture(scope="module")
def counted(eng):
    clips = C.count_clips()
    return clips, _stft(eng, clips)


def test_frame_counts_1_to_50_with_untrimmed_tails(eng, counted):
    clips, (lm, ph, foff) = counted
    assert 0 in C.count_tails() and 159 in C.count_tails()
    assert foff == C.offsets(range(1, C.COUNT_CLIPS + 1))            # nhans_num_frames ignores the tail
    ratio = C.yardstick_ratio("count", clips)
    bad, rel = [], 0.0
    for i, w in enumerate(clips):
        v = C.check_analysis("count", i, lm[foff[i]:foff[i + 1]], ph[foff[i]:foff[i + 1]], w, ratio)
        rel = max(rel, v.rel)
        if not v.ok:
            bad.append(v.message)
    print("analysis frame counts: rel_hip %.3e  rel_cpu32 %.3e  hip/cpu32 %.2f" % (rel, ratio, rel / ratio))
    assert not bad, "\n".join(bad)


def test_without_phase_and_truncated_to_7_frames_the_same_bits(eng, counted):
    clips, (lm, ph, foff) = counted
    lm_np, none, foff_np = _stft(eng, clips, want_phase=False)
    assert none is None and foff_np == foff
    assert np.array_equal(lm_np.view(np.int32), lm.view(np.int32))
    # max_frames_per_clip = 7: a clip with fewer frames is refused (include/nhans_hip.h), so clips 6 .. 49 (T = 7 .. 50)
    with pytest.raises(hip.NhansError, match="clip 0 has 1 frames; 7 needed"):
        _stft(eng, clips, max_frames=7)
    for want_phase in (True, False):
        lm7, ph7, foff7 = _stft(eng, clips[6:], max_frames=7, want_phase=want_phase)
        assert foff7 == [7 * i for i in range(len(clips) - 6 + 1)]
        for j in range(len(clips) - 6):
            i = j + 6
            assert np.array_equal(lm7[7 * j:7 * j + 7].view(np.int32), lm[foff[i]:foff[i] + 7].view(np.int32)), i
            if want_phase:
                assert np.array_equal(ph7[7 * j:7 * j + 7].view(np.int32), ph[foff[i]:foff[i] + 7].view(np.int32)), i


# ---- inverse ------------------------------------------------------------------------------------------------------
def _istft(eng, spectra, gaps):
    """One ragged nhans_istft launch; clip i's output is followed by gaps[i] canary samples.  -> list of clip outputs."""
    foff = C.offsets([len(lm) for lm, _ in spectra])
    lens = [(len(lm) - 1) * C.HOP + C.WIN for lm, _ in spectra]
    ooff = [0]
    for n, g in zip(lens, gaps):
        ooff.append(ooff[-1] + n + g)
    lm_t = torch.from_numpy(np.concatenate([lm for lm, _ in spectra])).cuda()
    ph_t = torch.from_numpy(np.concatenate([ph for _, ph in spectra])).cuda()
    out = torch.full((ooff[-1],), CANARY, dtype=torch.float32, device="cuda")
    hip.check(eng.lib.nhans_istft(eng.handle, hip.ptr(lm_t), hip.ptr(ph_t), hip.i64_array(foff), len(spectra),
                                  hip.i64_array(ooff), hip.ptr(out), eng._stream()))
    out = out.cpu().numpy()
    res = []
    for i, n in enumerate(lens):
        res.append(out[ooff[i]:ooff[i] + n])
        assert (out[ooff[i] + n:ooff[i + 1]] == np.float32(CANARY)).all(), "samples behind clip %d's output were written" % i
    return res


def test_every_inverse_class_meets_the_bar(eng, analysis):
    classes, lm, ph, foff = analysis
    inv = C.inverse_classes(ph[foff[0]:foff[1]])
    outs = _istft(eng, [(l, p) for _, l, p in inv], [4] * len(inv))
    # Engine.istft lays the clips out back to back: the same bits
    e_out, e_off = eng.istft(torch.from_numpy(np.concatenate([l for _, l, _ in inv])).cuda(),
                             torch.from_numpy(np.concatenate([p for _, _, p in inv])).cuda(),
                             [C.FRAMES * i for i in range(len(inv) + 1)])
    e_out = e_out.cpu().numpy()
    assert e_off == [C.SAMPLES * i for i in range(len(inv) + 1)]
    bad = []
    for i, (name, l, p) in enumerate(inv):
        assert np.array_equal(e_out[e_off[i]:e_off[i + 1]].view(np.int32), outs[i].view(np.int32)), name
        # classes 7: outside [-pi, pi] the ABI promises the float32 rounding of the angle in revolutions, no more; the edge of
        # the full-accuracy range, +-float32(pi), is class 5, at the bar of all the others
        v = C.check_inverse(name, i, outs[i], l, p, phase_slack=C.PHASE_SLACK_7PI if name.startswith("7") else 0.0)
        print("inverse %-36s err_hip %.3e  err_cpu32 %.3e  max %.3e  hip/cpu32 %6.2f  hip/max %.2e  bar/max %.2e %s" % (
            name, v.err_hip, v.err_cpu32, v.m, v.err_hip / v.err_cpu32, v.err_hip / v.m, v.bar / v.m, "" if v.ok else "FAIL"))
        if not v.ok:
            bad.append(v.message)
    assert not bad, "\n".join(bad)


def test_inverse_frame_counts_1_to_50(eng):
    """Every position of the 22-hop runs and of their reach back to frame h0 - 2 on a clip's first, middle and last run;
    gaps of 4 and of 3 samples between the outputs: the 16-byte and the unaligned store path."""
    spectra = C.count_spectra()
    gaps = [4 if i % 4 < 2 else 3 for i in range(len(spectra))]
    outs = _istft(eng, spectra, gaps)
    bad, worst = [], (0.0, 0.0)
    for i, (l, p) in enumerate(spectra):
        v = C.check_inverse("count", i, outs[i], l, p)
        worst = max(worst, (v.err_hip / v.err_cpu32, v.err_hip / v.m))
        if not v.ok:
            bad.append(v.message)
    print("inverse frame counts: worst hip/cpu32 %.2f (hip/max %.2e)" % worst)
    assert not bad, "\n".join(bad)
