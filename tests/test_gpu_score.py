"""Scoring against a clean target on the device (score.hip, nhans_score_wave / nhans_score_rows) against the float64
definition nhans_amd.score.reference / reference_rows, within the bar of tests/score_checks.py; the figures' independence
of batch, offset and run, bit for bit; the edges; the fixture of the reference's own demo triples; Engine.score,
evaluate_utterance(scores=True) and the command line.  Every test prints its worst ratio to the bar (pytest -s)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import nhans_amd  # noqa: F401
from nhans_amd import apply, engine, score, spec, synth

import score_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wave(eng, pairs, pad_e=0, pad_t=0):
    """pairs scored in one call, the estimates' buffer starting with pad_e spare samples and the targets' with pad_t ->
    (records [n, 16] numpy, frames [F, 3] numpy)"""
    es, ts = [np.zeros(pad_e, np.float32)] + [p[0] for p in pairs], [np.zeros(pad_t, np.float32)] + [p[1] for p in pairs]
    eo, to = np.cumsum([0] + [len(x) for x in es]).tolist()[1:], np.cumsum([0] + [len(x) for x in ts]).tolist()[1:]
    rec, fr = eng.score_device(dev(np.concatenate(es)), eo, dev(np.concatenate(ts)), to, per_frame=True)
    return rec.cpu().numpy(), fr.cpu().numpy()


def as_dict(rec, frames=None):
    d = score.record(rec)
    if frames is not None:
        d["frames"] = frames
    return d


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_lengths_alone_and_batched_within_the_bar_and_bit_equal(eng):
    pairs = S.length_clips()
    alone = [wave(eng, [p]) for p in pairs]
    worst = {}
    for (rec, fr), (e, t), n in zip(alone, pairs, S.LENGTHS):
        assert fr.shape == (spec.frames_for_samples(n)[1], 3) and np.isnan(fr[:, 1:]).all()    # columns 1 - 2 untouched
        assert (rec[0, 12:] == 0.0).all()
        for k, v in S.wave_ratios(as_dict(rec[0], fr[:, 0]), e, t).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("score lengths: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst
    # all of them in one batch, every offset odd (estimates from element 1 on, targets from element 3 on)
    rec, fr = wave(eng, pairs, pad_e=1, pad_t=3)
    assert same_bits(rec, np.concatenate([a[0] for a in alone]))
    assert same_bits(fr[:, 0], np.concatenate([a[1][:, 0] for a in alone]))
    rec2, fr2 = wave(eng, pairs, pad_e=1, pad_t=3)
    assert same_bits(rec, rec2) and same_bits(fr, fr2)
    # another neighbourhood and another alignment: the same records
    rec3, _ = wave(eng, pairs[::-1], pad_e=2, pad_t=0)
    assert same_bits(rec3[::-1], rec)


def test_identity_and_edges(eng):
    e, t = S.clip(3 * S.TILE + 17, 40)
    td = dev(t)
    rec = eng.score_device(td, [0, len(t)], td, [0, len(t)]).cpu().numpy()[0]
    d = score.record(rec)
    assert d["alpha"] == 1.0 and d["Srr"] == 0.0 and d["Sdd"] == 0.0 and d["si_sdr_db"] == math.inf and d["snr_db"] == math.inf
    assert d["segsnr_db"] == 35.0 and d["frames_skipped"] == 0 and d["See"] == d["Stt"] == d["Set"]
    # silent frames, a wholly silent target, no sample at all, unequal lengths: one batch
    es, ts = S.silent_frames_clip()
    z = np.zeros(1000, np.float32)
    pairs = [(es, ts), (e[:1000], z), (e[:0], t[:0]), (e, t[:1500]), (e[:700], t)]
    rec, fr = wave(eng, pairs, pad_e=1)
    nf = [spec.frames_for_samples(min(len(a), len(b)))[1] for a, b in pairs]
    assert fr.shape[0] == sum(nf) and nf == [11, 4, 0, 7, 2]
    d0 = as_dict(rec[0], fr[:11, 0])
    assert (d0["frames_counted"], d0["frames_skipped"]) == (8, 3) and np.isnan(fr[2:5, 0]).all() and (fr[8:11, 0] == 35.0).all()
    assert max(S.wave_ratios(d0, es, ts).values()) <= 1.0
    d1 = score.record(rec[1])
    assert d1["alpha"] == 0.0 and d1["Stt"] == 0.0 and math.isnan(d1["snr_db"]) and math.isnan(d1["si_sdr_db"])
    assert math.isnan(d1["segsnr_db"]) and (d1["frames_counted"], d1["frames_skipped"]) == (0, 4) and np.isnan(fr[11:15, 0]).all()
    assert max(S.wave_ratios(as_dict(rec[1]), e[:1000], z).values()) <= 1.0
    d2 = score.record(rec[2])
    assert [d2[k] for k in ("n", "See", "Stt", "Set", "Sdd", "alpha", "Srr", "frames_counted", "frames_skipped")] == [0] * 9
    assert math.isnan(d2["snr_db"]) and math.isnan(d2["si_sdr_db"]) and math.isnan(d2["segsnr_db"])
    for i, (a, b) in ((3, (e[:1500], t[:1500])), (4, (e[:700], t[:700]))):
        assert score.record(rec[i])["n"] == len(a)
        assert max(S.wave_ratios(as_dict(rec[i]), a, b).values()) <= 1.0
        assert same_bits(rec[i], wave(eng, [(a, b)])[0][0])                # the prefix, and nothing of what follows it
    # a frame at each clamp
    ec, tc = S.clamp_clip()
    rec, fr = wave(eng, [(ec, tc)])
    assert fr[0, 0] == -10.0 and fr[5, 0] == 35.0 and max(S.wave_ratios(as_dict(rec[0], fr[:, 0]), ec, tc).values()) <= 1.0
    # a non-finite sample propagates
    bad = e.copy()
    bad[5] = np.nan
    d = score.record(wave(eng, [(bad, t)])[0][0])
    assert math.isnan(d["See"]) and math.isnan(d["snr_db"]) and math.isnan(d["si_sdr_db"]) and math.isnan(d["segsnr_db"])


def test_rows_within_the_bar_and_bit_equal(eng):
    counts = S.ROW_COUNTS
    Es, Ts = [S.uniform_rows(n, 10 + n) for n in counts], [S.uniform_rows(n, 50 + n) for n in counts]
    lo, hi = S.edge_rows(17)
    Es, Ts, counts = Es + [lo, hi], Ts + [hi, lo], counts + [17, 17]
    off = np.cumsum([0] + counts).tolist()
    rec, fr = eng.score_rows(dev(np.concatenate(Es)), dev(np.concatenate(Ts)), off, per_frame=True)
    rec, fr = rec.cpu().numpy(), fr.cpu().numpy()
    assert fr.shape == (off[-1], 3) and np.isnan(fr[:, 0]).all() and (rec[:, 3:] == 0.0).all()
    worst = {}
    for i, (E, T) in enumerate(zip(Es, Ts)):
        got = dict(score.row_record(rec[i]), per_frame=fr[off[i]:off[i + 1], 1:])
        for k, v in S.rows_ratios(got, E, T).items():
            worst[k] = max(worst.get(k, 0.0), v)
        one = eng.score_rows(dev(E), dev(T), [0, counts[i]]).cpu().numpy() if counts[i] else None
        if one is not None:
            assert same_bits(one[0], rec[i])
    print("score rows: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst
    d = score.row_record(rec[0])
    assert d["frames"] == 0 and math.isnan(d["loss"]) and math.isnan(d["lsd_db"])
    again = eng.score_rows(dev(np.concatenate(Es)), dev(np.concatenate(Ts)), off).cpu().numpy()
    assert same_bits(again, rec)
    # completing score_device's per-frame tensor in place
    e, t = S.clip(400 + 160 * 16, 60)
    _, fr = eng.score_device(dev(e), [0, len(e)], dev(t), [0, len(t)], per_frame=True)
    _, fr2 = eng.score_rows(dev(Es[4]), dev(Ts[4]), [0, 17], per_frame=True, frames_out=fr)
    assert fr2 is fr and not torch.isnan(fr).any()


def test_fixture_of_the_reference_demo_triples(eng):
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    keys = [str(k) for k in g["score_keys"]]
    worst = {}
    for ex in ("example2", "example3"):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        got = eng.score([sig["denoised"], sig["mixed"], sig["target"]], [sig["target"]] * 3)
        for name, rec in zip(("denoised", "mixed"), got):
            stored = dict(zip(keys, g["%s_%s_scores" % (ex, name)]))
            _, bar, _ = S.wave_bar(sig[name], sig["target"])
            for k in S.WAVE_FIGURES:
                worst[k] = max(worst.get(k, 0.0), S.ratio(rec[k], stored[k], bar[k]))
            assert (rec["n"], rec["frames_counted"], rec["frames_skipped"]) == (stored["n"], stored["frames_counted"], 0)
        assert got[2]["si_sdr_db"] == math.inf and got[2]["loss"] == 0.0 and got[2]["lsd_db"] == 0.0
        # the row figures are those of the device's own float32 rows (the stored ones are of float64 rows of the same signals,
        # an STFT apart): held to the definition on the rows the device scored
        flat = dev(np.concatenate([sig["denoised"], sig["mixed"], sig["target"]]))
        n = len(sig["target"])
        lm, _ = eng.stft_features(flat, [0, n, 2 * n, 3 * n], want_phase=False)
        lm = lm.cpu().numpy().reshape(3, -1, spec.BINS)
        for i in (0, 1):
            for k, v in S.rows_ratios({k: got[i][k] for k in score.ROW_FIELDS}, lm[i], lm[2]).items():
                worst[k] = max(worst.get(k, 0.0), v)
        imp = score.improvement(got[1], got[0])
        assert imp["si_sdr_i"] > 0 and imp["snr_i"] > 0 and imp["segsnr_i"] > 0 and imp["loss_ratio"] < 1, imp
        assert got[0]["lsd_db"] < got[1]["lsd_db"]
    print("score fixture: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


def test_engine_score_is_the_two_device_calls(eng):
    pairs = [S.clip(n, 80 + i) for i, n in enumerate((400, 1999, 2 * S.TILE + 1))]
    pairs.append((pairs[0][0], pairs[1][1]))                                    # unequal lengths: the prefix
    got = eng.score([p[0] for p in pairs], [p[1] for p in pairs], per_frame=True)
    cut = [(e[:min(len(e), len(t))], t[:min(len(e), len(t))]) for e, t in pairs]
    off = np.cumsum([0] + [len(e) for e, _ in cut]).tolist()
    ed, td = dev(np.concatenate([e for e, _ in cut])), dev(np.concatenate([t for _, t in cut]))
    rec, fr = eng.score_device(ed, off, td, off, per_frame=True)
    le, _ = eng.stft_features(ed, off, want_phase=False)
    lt, _ = eng.stft_features(td, off, want_phase=False)
    foff = np.cumsum([0] + [spec.frames_for_samples(len(e))[1] for e, _ in cut]).tolist()
    rrec, fr = eng.score_rows(le, lt, foff, per_frame=True, frames_out=fr)
    rec, rrec, fr = rec.cpu().numpy(), rrec.cpu().numpy(), fr.cpu().numpy()
    worst = 0.0
    for i, g in enumerate(got):
        want = dict(score.record(rec[i]), **score.row_record(rrec[i]))
        assert {k: g[k] for k in want} == want
        assert same_bits(g["per_frame"], fr[foff[i]:foff[i + 1]])
        worst = max(worst, max(S.rows_ratios(dict(score.row_record(rrec[i]), per_frame=fr[foff[i]:foff[i + 1], 1:]),
                                             le[foff[i]:foff[i + 1]].cpu().numpy(), lt[foff[i]:foff[i + 1]].cpu().numpy()).values()))
    print("score engine: worst row ratio to the bar %.3f" % worst)
    assert worst <= 1.0
    assert eng.score([], []) == []


def test_evaluate_utterance_scores(eng, tmp_path):
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        paths = {}
        for name, sig in (("speech", synth.mixture(30, 2.6)), ("pos", synth.noise_context(30, 1.0)),
                          ("neg", synth.speaker_context(30, 3.0))):
            paths[name] = str(tmp_path / (name + ".wav"))
            wavfile.write(paths[name], 16000, sig)
        loss0 = apply.evaluate_utterance(paths["speech"], paths["pos"], paths["neg"], str(tmp_path / "a"), "nhans", 1)
        loss, sc = apply.evaluate_utterance(paths["speech"], paths["pos"], paths["neg"], str(tmp_path / "b"), "nhans", 1, scores=True)
        assert loss == loss0 and isinstance(loss0, float)
        for name in sorted(os.listdir(str(tmp_path / "a"))):
            assert open(str(tmp_path / "a" / name), "rb").read() == open(str(tmp_path / "b" / name), "rb").read()
        rows = sc["rows"]
        for name in ("denoised", "mixed"):
            r = eng.score_rows(dev(rows[name]), dev(rows["target"]), [0, len(rows["target"])]).cpu().numpy()[0]
            assert score.row_record(r) == {k: sc[name][k] for k in score.ROW_FIELDS}
            assert max(S.rows_ratios(score.row_record(r), rows[name], rows["target"]).values()) <= 1.0
            assert all(math.isfinite(sc[name][k]) for k in score.FIGURES)
        # the float32 loss of the default call and the double one of the same rows: float32 rounding of 201 + frames terms apart
        assert sc["denoised"]["loss"] == pytest.approx(loss, rel=(spec.BINS + len(rows["target"]) + 8) * 2.0 ** -24)
        assert set(sc["improvement"]) == {"si_sdr_i", "snr_i", "segsnr_i", "loss_ratio"}
    finally:
        apply._engines.pop("denoiser", None)


def test_cli_scores_and_leaves_the_audio_alone(eng, tmp_path, capsys):
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        clean = synth.mixture(41, 1.0)
        noise = synth.noise_context(41, 1.0)
        mixed = (clean.astype(np.int32) // 2 + noise[:len(clean)].astype(np.int32) // 4).astype(np.int16)
        ind, tgd, negd = tmp_path / "in", tmp_path / "tgt", tmp_path / "neg"
        for d in (ind, tgd, negd):
            d.mkdir()
        for name, k in (("a.wav", len(mixed)), ("b.wav", len(mixed) - 1000)):
            wavfile.write(str(ind / name), 16000, mixed[:k])
            wavfile.write(str(tgd / name), 16000, (clean // 2)[:k])
            wavfile.write(str(negd / name), 16000, noise)
        common = ["--pos", str(tmp_path / "Silent.wav"), "--weights", "synthetic"]
        # file mode, JSON on stdout
        apply.main(["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav"), "--output", str(tmp_path / "plain.wav")] + common)
        capsys.readouterr()
        apply.main(["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav"), "--output", str(tmp_path / "scored.wav"),
                    "--score_against", str(tgd / "a.wav")] + common)
        text = capsys.readouterr().out
        res = json.loads(text[text.index("{"):])
        (path, rec), = res["files"].items()
        assert path == str(ind / "a.wav") and res["skipped"] == [] and "mean" not in res
        assert set(rec) == {"denoised", "mixed", "improvement"}
        for k in ("denoised", "mixed"):
            assert set(score.FIELDS) | {"loss", "lsd_db", "frames"} <= set(rec[k])
            assert all(math.isfinite(rec[k][f]) for f in score.FIGURES), rec[k]
        assert rec["improvement"]["si_sdr_i"] == rec["denoised"]["si_sdr_db"] - rec["mixed"]["si_sdr_db"]
        for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
            assert open(str(tmp_path / ("plain" + tail)), "rb").read() == open(str(tmp_path / ("scored" + tail)), "rb").read()
        # directory mode, JSON to a file, with the means
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "o1")] + common)
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "o2"), "--score_against", str(tgd),
                    "--score_out", str(tmp_path / "s.json")] + common)
        res = json.load(open(str(tmp_path / "s.json")))
        assert sorted(res["files"]) == [str(ind / "a.wav"), str(ind / "b.wav")]
        assert all(math.isfinite(f[k][fig]) for f in res["files"].values() for k in ("denoised", "mixed") for fig in score.FIGURES)
        m = res["mean"]["denoised"]["snr_db"]
        assert m == pytest.approx(np.mean([f["denoised"]["snr_db"] for f in res["files"].values()]), rel=1e-15)
        assert set(res["mean"]) == {"denoised", "mixed", "improvement"}
        assert sorted(os.listdir(str(tmp_path / "o1"))) == sorted(os.listdir(str(tmp_path / "o2")))
        for name in os.listdir(str(tmp_path / "o1")):
            assert open(str(tmp_path / "o1" / name), "rb").read() == open(str(tmp_path / "o2" / name), "rb").read()
    finally:
        apply._engines.pop("denoiser", None)
        for k in ("score_against", "score_out"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.input, apply.FLAGS.output, apply.FLAGS.neg, apply.FLAGS.pos = (apply.Flags.input, apply.Flags.output,
                                                                                    apply.Flags.neg, apply.Flags.pos)
        apply.FLAGS.weights = apply.Flags.weights
