"""Mixing at a chosen SNR on the device (mix.hip, nhans_mix) against the rule restated with explicit dtypes
(tests/mix_checks.py), bit for bit: every output and every field of the record, alone and batched, at odd offsets, run
after run; the launches the profile shows; the demo and evaluation entry points with mix_on="gpu"; and
apply.evaluate_corpus against evaluate_utterance(scores=True) job by job."""
import ctypes
import math
import os
import warnings

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import apply, context, engine, hip, mixing, score, spec, synth

import mix_checks as M

pytestmark = pytest.mark.gpu
T = hip.MIX_TILE


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_s(weights_separator, lib_built):
    e = engine.Engine("separator", weights_separator)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(eng, speech, noises, jobs, pad_s=0, pad_n=0, want=("mixture", "target", "keep", "drop")):
    """jobs over the clips, the speech buffer beginning with pad_s spare samples and the noise buffer with pad_n ->
    (dict name -> list of per-job float32 arrays, records [jobs, 8])"""
    sf, soff = context.flat([np.zeros(pad_s, np.float32)] + list(speech))
    nf, noff = context.flat([np.zeros(pad_n, np.float32)] + list(noises))
    shifted = [(j[0] + 1, j[1] + 1 if j[1] >= 0 else -1, j[2] + 1, j[3], j[4]) for j in jobs]
    sig, off, rec = eng.mix_device(dev(sf), soff, dev(nf), noff, shifted, want=want)
    host = {k: v.cpu().numpy() for k, v in sig.items()}
    return {k: [v[off[j]:off[j + 1]] for j in range(len(jobs))] for k, v in host.items()}, rec.cpu().numpy()


def check(sig, rec, j, ref, what):
    for k in M.OUTPUTS:
        if k in sig:
            assert M.same_bits(sig[k][j], ref[k]), (what, k, int(np.count_nonzero(M.bits(sig[k][j]) != M.bits(ref[k]))))
    for i, k in enumerate(M.FIELDS):
        assert float(rec[j][i]).hex() == float(ref[k]).hex(), (what, k, rec[j][i], ref[k])
    assert rec[j][7] == 0.0


@pytest.fixture(scope="module")
def material():
    """speech clips, noise clips, jobs and their references, computed once: every speech length against noises of 1, 7,
    n - 1, n and n + 5 samples, noises that wrap inside a tile and across a tile edge, both signs of SNR, the silent
    cases and the two-way form."""
    speech, noises, jobs = [], [], []

    def noise(m, seed, scale):
        noises.append(M.signal(m, seed, scale))
        return len(noises) - 1

    for n in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        speech.append(M.signal(n, 10 + n))
        si = len(speech) - 1
        ms = [m for m in (1, 7, n - 1, n, n + 5) if m >= 1]
        if n > T:
            ms += [700, T + 3]              # wraps inside a tile; wraps three samples past a tile edge
        ids = [noise(m, 1000 + 7 * n + k, (0.1, 0.7)[k % 2]) for k, m in enumerate(ms)]
        for k in range(len(ids)):
            jobs.append((si, ids[k], ids[(k + 1) % len(ids)], (-3, 5, 0)[k % 3], (8, -5)[k % 2]))
        jobs.append((si, -1, ids[-1], None, (3, -1)[si % 2]))                        # two-way
    # silence: a silent keep noise, a silent drop noise, silent speech, everything silent
    n = T + 1
    speech += [M.signal(n, 77), np.zeros(n, np.float32)]
    quiet, loud = noise(9, 0, 0.0), noise(n + 5, 78, 0.4)
    a, z = len(speech) - 2, len(speech) - 1
    jobs += [(a, quiet, loud, 3, -3), (a, loud, quiet, -3, 3), (z, loud, loud, 5, 0), (z, quiet, quiet, 0, 0), (a, -1, quiet, None, 3)]
    refs = [M.reference(speech[s], noises[k] if k >= 0 else None, noises[d], sk, sd, tile=T) for s, k, d, sk, sd in jobs]
    return speech, noises, jobs, refs


def test_bit_for_bit_against_the_restated_rule(eng, material):
    speech, noises, jobs, refs = material
    sig, rec = run(eng, speech, noises, jobs)
    assert rec.shape == (len(jobs), hip.MIX_FIELDS)
    for j, ref in enumerate(refs):
        check(sig, rec, j, ref, jobs[j])
    # the silent cases by hand
    silent = rec[-5:]
    assert silent[0][3] == 1.0 and silent[1][4] == 1.0 and silent[2][3] == 0.0 and silent[2][4] == 0.0
    assert tuple(silent[3][:7]) == (0.0, 0.0, 0.0, 1.0, 1.0, 0.0, float(np.float32(1e-6))) and not sig["mixture"][-2].any()
    # Context.mix: the same through one upload and one download, with the records by name
    few = [0, 5, len(jobs) - 5]
    sig2, recs = eng.mix(speech, noises, [jobs[j] for j in few])
    for i, j in enumerate(few):
        assert all(M.same_bits(sig2[k][i], refs[j][k]) for k in M.OUTPUTS)
        assert recs[i] == {k: refs[j][k] for k in mixing.RECORD_FIELDS}


def test_batch_offset_and_run_do_not_change_a_bit(eng, material):
    speech, noises, jobs, refs = material
    pick = [j for j in range(len(jobs)) if jobs[j][0] in (3, 6, 7)]              # 65, T + 1 and 2 T + 1 samples: several jobs each
    assert len(pick) >= 18
    alone = [run(eng, speech, noises, [jobs[j]]) for j in pick]
    # together, every clip at an odd element offset (speech from element 1 on, noise from element 3 on)
    sig, rec = run(eng, speech, noises, [jobs[j] for j in pick], pad_s=1, pad_n=3)
    again = run(eng, speech, noises, [jobs[j] for j in pick], pad_s=1, pad_n=3)
    for i, j in enumerate(pick):
        check(sig, rec, i, refs[j], jobs[j])
        for k in M.OUTPUTS:
            assert M.same_bits(alone[i][0][k][0], sig[k][i]) and M.same_bits(again[0][k][i], sig[k][i])
        assert M.same_bits(alone[i][1][0], rec[i]) and M.same_bits(again[1][i], rec[i])
    # another alignment and another neighbourhood
    sig3, rec3 = run(eng, speech, noises, [jobs[j] for j in pick[::-1]], pad_s=2, pad_n=1)
    assert M.same_bits(rec3[::-1], rec) and all(M.same_bits(sig3["drop"][len(pick) - 1 - i], sig["drop"][i]) for i in range(len(pick)))


def test_nullable_outputs(eng, material):
    speech, noises, jobs, refs = material
    pick = [j for j in range(len(jobs)) if jobs[j][0] == 7]
    sig, rec = run(eng, speech, noises, [jobs[j] for j in pick], pad_s=1, want=("mixture",))
    assert set(sig) == {"mixture"}
    for i, j in enumerate(pick):
        check(sig, rec, i, refs[j], jobs[j])
    # no record either: the C call itself
    sf, soff = context.flat(speech)
    nf, noff = context.flat(noises)
    args, off = context.mix_job_arrays([jobs[j] for j in pick], soff)
    st, nt, out = dev(sf), dev(nf), torch.zeros(off[-1], dtype=torch.float32, device="cuda")
    hip.check(eng.lib.nhans_mix(eng.handle, hip.ptr(st), hip.i64_array(soff), len(speech), hip.ptr(nt), hip.i64_array(noff),
                                len(noises), *args, len(pick), hip.ptr(out), None, None, None, hip.i64_array(off), None, eng._stream()))
    got = out.cpu().numpy()
    assert all(M.same_bits(got[off[i]:off[i + 1]], refs[j]["mixture"]) for i, j in enumerate(pick))
    sig, off, rec = eng.mix_device(st, soff, nt, noff, [])
    assert off == [0] and rec.shape == (0, hip.MIX_FIELDS) and sig["mixture"].numel() == 0


def test_launches_one_chain_per_distinct_clip_and_length(eng):
    speech = [M.signal(3 * T + 9, 1), M.signal(500, 2)]
    noises = [M.signal(900, 3, 0.2), M.signal(4 * T, 4, 0.5)]
    snrs = [(-3, 8), (0, 0), (3, 5), (5, -3), (8, 3)]
    jobs = [(0, 0, 1, a, b) for a, b in snrs] + [(1, 1, 0, 0, 0), (1, -1, 0, None, 3)]
    eng.set_option("profile", 1)
    eng.profile_reset()
    try:
        sig, rec = run(eng, speech, noises, jobs)
        eng.mix_device(dev(speech[0]), [0, len(speech[0])], dev(noises[0]), [0, 900], [])      # no job: nothing launched
        prof = {k: v for k, v in eng.profile().items() if v["calls"]}
    finally:
        eng.set_option("profile", 0)
    assert {k: v["calls"] for k, v in prof.items()} == {"mix_power": 1, "mix_combine": 1, "mix_finish": 1}
    # one chain per distinct (clip, fitted length): 3 for the five-SNR sweep, 3 for the two jobs on the short clip -- not 20
    fitted = 3 * (3 * T + 9) + 3 * 500
    assert prof["mix_power"]["flops"] == 2.0 * fitted and prof["mix_power"]["bytes"] == 4.0 * fitted + 8.0 * 6
    for j, (s, k, d, sk, sd) in enumerate(jobs):
        check(sig, rec, j, M.reference(speech[s], noises[k] if k >= 0 else None, noises[d], sk, sd, tile=T), jobs[j])
    assert len({rec[j][0] for j in range(5)}) == 1 and len({rec[j][3] for j in range(5)}) == 5      # one power, a gain per SNR


# ------------------------------------------------------------------------------ demo and evaluation entry points
def _write_triple(tmp_path, tag, i, samples):
    from scipy.io import wavfile
    paths = []
    for name, x in (("speech", synth.mixture(30 + i, 2.2)[:samples]), ("pos", synth.noise_context(30 + i, 1.0)),
                    ("neg", synth.speaker_context(30 + i, 3.0))):
        paths.append(str(tmp_path / ("%s%d_%s.wav" % (tag, i, name))))
        wavfile.write(paths[-1], 16000, x)
    return tuple(paths)


def _same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    for name in names:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    return names


def test_demo_and_evaluation_files_with_the_mixing_on_the_device(eng, eng_s, tmp_path):
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    eng_s.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    apply.set_engine("separator", eng_s)
    try:
        speech, pos, neg = _write_triple(tmp_path, "d", 0, 32400 + 3 * 160 + 70)            # trimmed to 204 frames
        spk = str(tmp_path / "spk.wav")
        wavfile.write(spk, 16000, synth.speaker_context(31, 2.2, low=False)[:32400 + 2 * 160 + 5])
        for on in ("host", "gpu"):
            d = tmp_path / on
            d.mkdir()
            apply.apply_demo(speech, pos, neg, str(d / "clip_output_demo.wav"), mix_on=on)
            apply.apply_demo_separator(spk, neg, str(d / "sep_output_demo.wav"), mix_on=on)
        assert len(_same_files(str(tmp_path / "host"), str(tmp_path / "gpu"))) == 4
        loss_h = apply.evaluate_utterance(speech, pos, neg, str(tmp_path / "eh"), "nhans", 3)
        loss_g = apply.evaluate_utterance(speech, pos, neg, str(tmp_path / "eg"), "nhans", 3, mix_on="gpu")
        assert loss_h == loss_g and len(_same_files(str(tmp_path / "eh"), str(tmp_path / "eg"))) == 5
        with pytest.raises(ValueError, match="mix_on"):
            apply.apply_demo(speech, pos, neg, str(tmp_path / "x_output_demo.wav"), mix_on="device")
    finally:
        apply._engines.pop("denoiser", None)
        apply._engines.pop("separator", None)


def _per_utterance(monkeypatch, triple, pair, dump_dir, lookahead=spec.LOOKAHEAD):
    """evaluate_utterance(scores=True) with its SNRs forced to `pair`"""
    eng = apply.get_engine("denoiser")
    with monkeypatch.context() as mp:
        mp.setattr(mixing, "eval_snrs", lambda path: pair)
        return eng._with_lookahead(lookahead, lambda: apply.evaluate_utterance(*triple, dump_dir, "nhans", 9, scores=True))


def _assert_job_equals_utterance(job, loss, sc):
    for name in ("denoised", "mixed"):
        for k in score.FIELDS + score.ROW_FIELDS:
            a, b = job[name][k], sc[name][k]
            assert float(a).hex() == float(b).hex(), (name, k, a, b)
    assert job["improvement"].keys() == sc["improvement"].keys()
    for k, v in sc["improvement"].items():
        assert float(job["improvement"][k]).hex() == float(v).hex() or (math.isnan(v) and math.isnan(job["improvement"][k]))
    # "loss" is the device's double figure of the denoised rows; evaluate_utterance's own return value is the float32 numpy
    # mean of the same rows: the float32 rounding of 201 + frames terms apart (tests/test_gpu_score.py holds the same bar)
    assert float(job["loss"]).hex() == float(sc["denoised"]["loss"]).hex()
    frames = sc["denoised"]["frames"]
    assert job["loss"] == pytest.approx(loss, rel=(spec.BINS + frames + 8) * 2.0 ** -24)


def test_evaluate_corpus_equals_the_per_utterance_route(eng, tmp_path, monkeypatch):
    """Three triples of 201, 202 and 205 frames (the network runs on 1, 2 and 5 frames) x two SNR pairs = 6 jobs in one
    pass: every score field, the improvement and the dumped files equal the per-utterance route's, bit for bit."""
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        triples = [_write_triple(tmp_path, "c", i, 32400 + 160 * extra + 33) for i, extra in enumerate((0, 1, 4))]
        pairs = [(-3, 5), (8, 0)]
        res = apply.evaluate_corpus(triples, snrs=pairs, dump_dir=str(tmp_path / "corpus"), modelname="nhans", step=9, per_frame=True)
        assert len(res) == 6 and [r["triple"] for r in res] == [t for t in triples for _ in pairs]
        assert [r["denoised"]["frames"] for r in res] == [1, 1, 2, 2, 5, 5]
        j = 0
        for triple in triples:
            for pair in pairs:
                loss, sc = _per_utterance(monkeypatch, triple, pair, str(tmp_path / "single"))
                assert (res[j]["snr_pos"], res[j]["snr_neg"]) == pair
                _assert_job_equals_utterance(res[j], loss, sc)
                assert res[j]["denoised"]["per_frame"].shape == (res[j]["denoised"]["frames"], 3)
                clean, pos, neg = mixing.read_triple(apply.read_wav, *triple)
                ref = M.reference(clean, pos, neg, pair[0], pair[1])
                assert res[j]["mix"] == {k: ref[k] for k in mixing.RECORD_FIELDS}
                j += 1
        assert len(_same_files(str(tmp_path / "corpus"), str(tmp_path / "single"))) == 30
        # without a dump and without per-frame figures: the same records; snrs=None: the triple's own pair
        plain = apply.evaluate_corpus(triples[:2], snrs=pairs)
        for a, b in zip(plain, res[:4]):
            assert all(float(a[n][k]).hex() == float(b[n][k]).hex() for n in ("denoised", "mixed") for k in score.FIELDS + score.ROW_FIELDS)
        own = apply.evaluate_corpus(triples[:1])
        assert len(own) == 1 and (own[0]["snr_pos"], own[0]["snr_neg"]) == mixing.eval_snrs(triples[0][0])
        assert apply.evaluate_corpus([]) == []
        # a triple whose mixture has no frame past the context is refused by name
        short = _write_triple(tmp_path, "s", 3, 32400 - 160)
        with pytest.raises(ValueError, match="s3_speech.wav.*200 frames"):
            apply.evaluate_corpus([triples[0], short], snrs=pairs)
    finally:
        apply._engines.pop("denoiser", None)


def test_evaluate_corpus_lookahead_and_saturation(eng, weights_denoiser, tmp_path, monkeypatch):
    eng.set_precision("f16x3")
    triples = [_write_triple(tmp_path, "l", i, 32400 + 160 * extra) for i, extra in enumerate((4, 2))]
    apply.set_engine("denoiser", eng)
    try:
        res = apply.evaluate_corpus(triples, snrs=[(0, 3)], lookahead=2)
        for job, triple in zip(res, triples):
            loss, sc = _per_utterance(monkeypatch, triple, (0, 3), str(tmp_path / "la"), lookahead=2)
            _assert_job_equals_utterance(job, loss, sc)
        full = apply.evaluate_corpus(triples[:1], snrs=[(0, 3)])
        assert full[0]["denoised"]["See"] != res[0]["denoised"]["See"]                  # the look-ahead is not ignored
    finally:
        apply._engines.pop("denoiser", None)
    # exponents forced to zero on weights whose first stored tensor overflows f16: the f32 redo, finite records, the precision
    # restored.  (conv1 of block 1 times 2^15 and the conv that reads it times 2^-15 -- a ReLU lies between, so what
    # leaves the block stays of the usual size and the waveforms finite; the other suites' recipe, conv1 times 3e5 alone,
    # drives the denoised rows to where exp() of them is infinite at any precision.)
    W = dict(weights_denoiser)
    W["resblock1_1_conv1/w"] = (W["resblock1_1_conv1/w"] * np.float32(2.0 ** 15)).astype(np.float32)
    W["resblock1_1_conv2/w"] = (W["resblock1_1_conv2/w"] * np.float32(2.0 ** -15)).astype(np.float32)
    e16 = engine.Engine("denoiser", W, precision="f16x3")
    apply.set_engine("denoiser", e16)
    try:
        e16.set_activation_exponents([0] * hip.NUM_ACTIVATIONS)
        with pytest.warns(UserWarning, match="f16 range"):
            sat = apply.evaluate_corpus(triples, snrs=[(0, 3)])
        # (a tensor reached 65504 ~ 2^16 and the exponents keep the stored maximum 2^8 below the f16 limit: at least 8)
        assert e16.precision == "f16x3" and max(e16.activation_exponents()) >= 8
        for job in sat:
            for name in ("denoised", "mixed"):
                assert all(math.isfinite(job[name][k]) for k in ("See", "Stt", "Sdd", "snr_db", "si_sdr_db", "segsnr_db", "loss", "lsd_db")), job[name]
            assert all(math.isfinite(v) for v in job["mix"].values())
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            apply.evaluate_corpus(triples[:1], snrs=[(0, 3)])                           # the raised exponents fit: no second redo
    finally:
        apply._engines.pop("denoiser", None)
        e16.close()
