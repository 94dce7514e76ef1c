"""Phase refinement on the device (phase.hip, nhans_phase_project / nhans_phase_refine) against the float64 definition
nhans_amd.phase within the bar of tests/phase_checks.py: one projection on every class and shape, teacher-forced over eight
iterations, the bits' independence of batch, position and run, the refinement inside nhans_enhance_clips, the memory
contract, the free-running iteration, and the value on the demo triples.  Every test prints its figures (pytest -s)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import apply, engine, hip, mixing, phase, score, spec, synth

import memory_checks as M
import phase_checks as P

pytestmark = pytest.mark.gpu

CLASSES = P.classes()


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def project(eng, clips, inc=False):
    """clips: [(lm, t)] in one call -> [d per clip] (and the inconsistencies)"""
    off = P.offsets(len(c[0]) for c in clips)
    out = eng.phase_project_rows(dev(np.concatenate([c[0] for c in clips])), dev(np.concatenate([c[1] for c in clips])), off, inc=inc)
    d = (out[0] if inc else out).cpu().numpy()
    ds = [d[off[i]:off[i + 1]] for i in range(len(clips))]
    return (ds, out[1].cpu().numpy()) if inc else ds


def refine(eng, clips, iters, alpha=0.0):
    """clips: [(lm, ph)] in one call -> ([phase per clip], inc [n, iters])"""
    off = P.offsets(len(c[0]) for c in clips)
    ph, inc = eng.phase_refine_rows(dev(np.concatenate([c[0] for c in clips])), dev(np.concatenate([c[1] for c in clips])), off, iters, alpha,
                                    inc=True)
    ph = ph.cpu().numpy()
    return [ph[off[i]:off[i + 1]] for i in range(len(clips))], inc.cpu().numpy()


def test_one_projection_on_every_class_and_shape(eng):
    """Every class in ONE ragged call (T = 1 ... 5, R - 1, R, R + 1, 2 R + 1, the demo clip, the level classes, the state
    with zero and sub-normal entries), every frame and bin under its class's bar; inc against the definition."""
    ds, inc = project(eng, [(lm, t) for _, lm, t in CLASSES], inc=True)
    for (name, lm, t), d, ic in zip(CLASSES, ds, inc):
        ref = P.reference64(lm, t)
        ratio = P.yardstick_ratio(name, lm, t)
        v = P.check_project(name, d, lm, t, ratio, ref=ref)
        want = phase.inconsistency(lm, ref)
        print("%-32s device %.3e  cpu32 %.3e  of the scale; inc %.6e for %.6e" % (name, v.rel, ratio, ic, want))
        assert v.ok, v.message
        # (|d| - A)^2 moves by 2 | |d| - A | err: K ratio scale per bin against terms of the scale's square
        assert abs(ic - want) <= 1e-4 * want, (name, ic, want)


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_teacher_forced_over_eight_iterations(eng, alpha):
    """At n = 0 ... 7 the float64 state of the reference, rounded to float32, goes through one projection of the device:
    both sides take the same t, so every frame is held to the one-projection bar."""
    lm, ph = P.uniform_case(30, 4030)
    ref = phase.reference(lm, ph, 8, alpha, states=True)
    worst = 0.0
    for n in range(8):
        t = ref["t"][n].astype(np.complex64)
        ratio = P.yardstick_ratio(("forced", alpha, n), lm, t)
        v = P.check_project("forced alpha %g n %d" % (alpha, n), project(eng, [(lm, t)])[0], lm, t, ratio)
        worst = max(worst, v.rel / ratio)
        assert v.ok, v.message
    print("alpha %g: worst device / cpu32 over the iterations %.2f (bar %g)" % (alpha, worst, P.K))


def test_bits_alone_batched_moved_and_again(eng):
    cases = [(lm, P.uniform_case(len(lm), 77 + len(lm))[1]) for name, lm, _ in CLASSES if name.startswith("uniform")]
    N = 8
    alone = [refine(eng, [c], N, 0.5) for c in cases]
    batch = refine(eng, cases, N, 0.5)
    again = refine(eng, cases, N, 0.5)
    order = list(range(len(cases)))[::-1]
    moved = refine(eng, [cases[i] for i in order], N, 0.5)
    for i, (ph_a, inc_a) in enumerate(alone):
        assert bits(ph_a[0]) == bits(batch[0][i]) == bits(again[0][i]) == bits(moved[0][order.index(i)]), "clip %d" % i
        assert bits(inc_a[0]) == bits(batch[1][i]) == bits(again[1][i]) == bits(moved[1][order.index(i)]), "clip %d" % i
        assert np.isfinite(inc_a).all() and np.abs(ph_a[0]).max() <= np.float32(np.pi)
    short = refine(eng, cases, 3, 0.5)
    assert bits(short[1]) == bits(batch[1][:, :3])
    zero = refine(eng, cases, 0)
    for (lm, ph), out in zip(cases, zero[0]):
        assert bits(out) == bits(ph)
    assert zero[1].shape == (len(cases), 0)


def test_two_plain_iterations_are_two_projections(eng):
    """alpha = 0 runs without the d plane: the state after two iterations is one projection after another."""
    lm, ph = P.uniform_case(P.RUN + 1, 505)
    out, _ = refine(eng, [(lm, ph)], 2)
    t0 = P.unit_state(ph)
    d0 = project(eng, [(lm, t0)])[0]
    d1 = project(eng, [(lm, d0)])[0]
    # (the device forms t_0 with its own sine and cosine: the comparison is through the definition's bar, not the bits)
    want = np.angle(d1.astype(np.complex128))
    diff = np.abs(np.angle(np.exp(1j * (out[0].astype(np.float64) - want))))
    loud = np.abs(d1) > 1e-2 * np.exp(lm.astype(np.float64))
    print("two plain iterations against two projections: %.3e rad at the loud bins" % diff[loud].max())
    assert diff[loud].max() < 1e-4


def _clips(n_frames):
    """mixtures of n_frames[i] whole frames and two conditioning recordings each, float32 in [-1, 1]"""
    f32 = lambda x: (x.astype(np.float32) / np.float32(32768.0))
    sig = [f32(synth.mixture(i, seconds=1.0))[:spec.WIN + spec.HOP * (t - 1)] for i, t in enumerate(n_frames)]
    return sig, [f32(synth.noise_context(i)) for i in range(len(n_frames))], [f32(synth.noise_context(10 + i)) for i in range(len(n_frames))]


def test_enhance_clips_with_and_without_iterations(eng):
    mixes, ca, cb = _clips([P.RUN + 3, 2 * P.RUN + 1])
    base = eng.enhance(mixes, ca, cb, want_mixed=True, taps=True)
    eng.set_option("phase_iters", 0)
    zero = eng.enhance(mixes, ca, cb, want_mixed=True, taps=True)
    four = eng.enhance(mixes, ca, cb, want_mixed=True, taps=True, phase_iters=4, phase_alpha=0.25)
    after = eng.enhance(mixes, ca, cb, want_mixed=True, taps=True)
    for k in ("logmag", "phase", "logits", "emb"):
        assert bits(base[k]) == bits(zero[k]) == bits(four[k]) == bits(after[k]), k
    for i in range(len(mixes)):
        assert bits(base["denoised_wav"][i]) == bits(zero["denoised_wav"][i]) == bits(after["denoised_wav"][i])
        assert bits(base["mixed_wav"][i]) == bits(four["mixed_wav"][i])
        assert bits(base["denoised_wav"][i]) != bits(four["denoised_wav"][i])
    # the N = 4 waveform: nhans_istft over nhans_phase_refine of the call's own denoised rows and phase tap
    foff = P.offsets(int(eng.lib.nhans_num_frames(len(m))) for m in mixes)
    lm, ph, emb = dev(four["logmag"]), dev(four["phase"]), dev(four["emb"])
    _, den = eng.mask_net(lm, foff, emb[:len(mixes)], emb[len(mixes):])
    wav, ooff = eng.istft(den, eng.phase_refine_rows(den, ph, foff, 4, 0.25), foff)
    wav = wav.cpu().numpy()
    for i in range(len(mixes)):
        assert bits(wav[ooff[i]:ooff[i + 1]]) == bits(four["denoised_wav"][i]), "clip %d" % i


def test_inputs_are_read_only_and_nothing_is_written_beside_the_outputs(eng):
    cases = [(lm, P.uniform_case(len(lm), 31 + len(lm))[1]) for name, lm, _ in CLASSES if name.startswith("uniform")]
    off = P.offsets(len(c[0]) for c in cases)
    F, n, N = off[-1], len(cases), 3
    lm_t, ph_t = dev(np.concatenate([c[0] for c in cases])), dev(np.concatenate([c[1] for c in cases]))
    st_t = dev(P.unit_state(np.concatenate([c[1] for c in cases])))
    before = [bits(x.cpu().numpy()) for x in (lm_t, ph_t, st_t)]
    runs = {"phase": [], "inc": [], "d": [], "inc1": []}
    for which in (0, 1):
        g = {"phase": M.Guarded("f32", F * P.BINS, align=1, which=which, device="cuda"),
             "inc": M.Guarded("f64", n * N, align=1, which=which, device="cuda"),
             "d": M.Guarded("f32", 2 * F * P.BINS, align=2, which=which, device="cuda"),
             "inc1": M.Guarded("f64", n, which=which, device="cuda")}
        p = lambda k: ctypes.c_void_p(g[k].ptr)
        hip.check(eng.lib.nhans_phase_refine(eng.handle, hip.ptr(lm_t), hip.ptr(ph_t), hip.i64_array(off), n, N, 0.5, p("phase"), p("inc"),
                                             eng._stream()))
        hip.check(eng.lib.nhans_phase_project(eng.handle, hip.ptr(lm_t), hip.ptr(torch.view_as_real(st_t)), hip.i64_array(off), n, p("d"),
                                              p("inc1"), eng._stream()))
        torch.cuda.synchronize()
        for k in g:
            runs[k].append(g[k])
    for k, size in (("phase", F * P.BINS), ("inc", n * N), ("d", 2 * F * P.BINS), ("inc1", n)):
        fs = M.findings(runs[k], np.ones(size, dtype=bool))
        assert not fs, k + ": " + M.report(fs)
    assert before == [bits(x.cpu().numpy()) for x in (lm_t, ph_t, st_t)]
    # the guarded outputs are what the tensors of the binding receive
    want, winc = refine(eng, cases, N, 0.5)
    assert bits(runs["phase"][0].region()) == bits(np.concatenate(want)) and bits(runs["inc"][0].region()) == bits(winc)


def test_refusals_name_the_clip_and_write_nothing(eng):
    lm, ph = P.uniform_case(4, 5)
    lm_t, ph_t = dev(lm), dev(ph)
    out = torch.full_like(ph_t, 7.0)
    call = lambda off, n, iters, alpha, a=lm_t, b=ph_t, o=out: eng.lib.nhans_phase_refine(
        eng.handle, hip.ptr(a), hip.ptr(b), hip.i64_array(off), n, iters, alpha, hip.ptr(o), None, eng._stream())
    for args, word in (((([0, 4]), 1, -1, 0.0), "iters"), (([0, 4], 1, 257, 0.0), "iters"), (([0, 4], 1, 2, 1.0), "alpha"),
                       (([0, 4], 1, 2, -0.5), "alpha"), (([0, 2, 2, 4], 3, 2, 0.0), "clip 1 has no frame"),
                       (([0, 3, 2], 2, 2, 0.0), "clip 1"), (([0, 4], -1, 2, 0.0), "negative")):
        rc = call(*args)
        assert rc == -1 and word in eng.lib.nhans_last_error().decode(), (args, eng.lib.nhans_last_error())
    for a, b, o in ((None, ph_t, out), (lm_t, None, out), (lm_t, ph_t, None)):
        assert call([0, 4], 1, 2, 0.0, a, b, o) == -1 and "null" in eng.lib.nhans_last_error().decode()
    st = dev(P.unit_state(ph))
    assert eng.lib.nhans_phase_project(eng.handle, hip.ptr(lm_t), hip.ptr(torch.view_as_real(st)), hip.i64_array([0, 4]), 1,
                                       hip.ptr(torch.view_as_real(st)), None, eng._stream()) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call([0], 0, 2, 0.0) == 0                        # no clip: nothing to do
    with pytest.raises(hip.NhansError):
        eng.set_option("phase_iters", 257)
    assert eng.lib.nhans_phase_set_alpha(eng.handle, 1.0) == -1 and eng.lib.nhans_phase_set_alpha(eng.handle, 0.0) == 0


FREE = [("uniform 30", lambda: P.uniform_case(30, 4030)), ("example2 magnitudes", lambda: P.demo_rows("example2")[:2])]


@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("name,make", FREE, ids=[f[0] for f in FREE])
def test_free_running_eight_iterations(eng, name, make, alpha):
    """inc[n] and the final waveform of N = 8 against the float64 iteration, K times what the float32 restatement's own
    free-running iteration differs from it by (tests/phase_checks.py)."""
    lm, ph = make()
    ref, inc_rel, wave_abs, wave_max = P.free_running_yardstick(lm, ph, 8, alpha)
    (out,), inc = refine(eng, [(lm, ph)], 8, alpha)
    wav, _ = eng.istft(dev(lm), dev(out), [0, len(lm)])
    wav = wav.cpu().numpy()
    d_inc = float((np.abs(inc[0] - ref["inc"]) / ref["inc"]).max())
    d_wav = float(np.abs(wav.astype(np.float64) - ref["wave"]).max())
    print("%s alpha %g: inc rel device %.3e cpu32 %.3e; wave device %.3e cpu32 %.3e of peak %.3e" % (
        name, alpha, d_inc, inc_rel, d_wav, wave_abs, wave_max))
    assert inc_rel < P.ILL and wave_abs < P.ILL * wave_max, "the restatement is no yardstick here: see the teacher-forced test"
    assert d_inc <= P.K * inc_rel, (d_inc, inc_rel)
    assert d_wav <= P.K * wave_abs, (d_wav, wave_abs)


def test_phase_ceiling_matches_the_definition_on_the_demo_triples(eng):
    for ex in ("example2", "example3"):
        lm, ph, tgt, mix = P.demo_rows(ex)
        recs = apply.phase_ceiling(eng, mix, tgt, iters=(0, 8, 32))
        row = []
        for r in recs:
            want = phase.si_sdr(phase.reference(lm, ph, r["iters"])["wave"], tgt)
            row.append((r["iters"], r["si_sdr_db"], want))
            assert abs(r["si_sdr_db"] - want) < 0.05, (ex, r["iters"], r["si_sdr_db"], want)
            assert len(r["inc"]) == r["iters"]
        print(ex, "mixture %.2f dB;" % phase.si_sdr(mix, tgt), "  ".join("N=%d: %.2f (f64 %.2f)" % x for x in row))
        assert recs[1]["si_sdr_db"] > recs[0]["si_sdr_db"] + 1.0


def _write_triple(tmp_path, i, samples):
    from scipy.io import wavfile
    paths = []
    for name, x in (("speech", synth.mixture(40 + i, 2.2)[:samples]), ("pos", synth.noise_context(40 + i, 1.0)),
                    ("neg", synth.speaker_context(40 + i, 3.0))):
        paths.append(str(tmp_path / ("p%d_%s.wav" % (i, name))))
        wavfile.write(paths[-1], 16000, x)
    return tuple(paths)


def test_evaluation_routes_refine_alike_and_leave_the_rest_alone(eng, tmp_path, monkeypatch):
    """evaluate_corpus(phase_iters=3) equals evaluate_utterance(phase_iters=3) job by job, figures and files bit for bit; against
    the route without iterations only the denoised waveform -- its file and its waveform figures -- differs."""
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        triples = [_write_triple(tmp_path, i, 32400 + 160 * extra + 33) for i, extra in enumerate((P.RUN + 2, 4))]
        monkeypatch.setattr(mixing, "eval_snrs", lambda path: (3, 0))
        res = apply.evaluate_corpus(triples, snrs=[(3, 0)], dump_dir=str(tmp_path / "corpus"), phase_iters=3, phase_alpha=0.25)
        plain = apply.evaluate_corpus(triples, snrs=[(3, 0)], dump_dir=str(tmp_path / "plain"))
        for job, base, triple in zip(res, plain, triples):
            loss, sc = apply.evaluate_utterance(*triple, str(tmp_path / "single"), scores=True, phase_iters=3, phase_alpha=0.25)
            for name in ("denoised", "mixed"):
                for k in score.FIELDS + score.ROW_FIELDS:
                    assert float(job[name][k]).hex() == float(sc[name][k]).hex(), (name, k)
            for k in score.FIELDS + score.ROW_FIELDS:
                assert float(job["mixed"][k]).hex() == float(base["mixed"][k]).hex(), k
            for k in score.ROW_FIELDS:
                assert float(job["denoised"][k]).hex() == float(base["denoised"][k]).hex(), k
            assert job["denoised"]["si_sdr_db"] != base["denoised"]["si_sdr_db"]
        names = sorted(os.listdir(tmp_path / "corpus"))
        assert names == sorted(os.listdir(tmp_path / "single")) == sorted(os.listdir(tmp_path / "plain")) and len(names) == 10
        for name in names:
            got = open(tmp_path / "corpus" / name, "rb").read()
            assert got == open(tmp_path / "single" / name, "rb").read(), name
            assert (got == open(tmp_path / "plain" / name, "rb").read()) == (not name.endswith("denoised.wav")), name
    finally:
        apply._engines.pop("denoiser", None)
