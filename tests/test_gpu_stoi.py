"""STOI and extended STOI on the device (stoi.hip, nhans_stoi) against the float64 definition
nhans_amd.score.stoi_reference on identical 10 kHz input, within the bar of tests/stoi_checks.py; the figures'
independence of batch, offset and run, bit for bit; the edges; the 16 -> 10 kHz conversion against
scipy.signal.resample_poly; the fixture of the reference's own demo triples; Context.score(stoi=True), evaluate_utterance,
evaluate_corpus and the command line.  Every test prints its worst ratio to the bar (pytest -s)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import nhans_amd  # noqa: F401
from nhans_amd import apply, engine, hip, mixing, score, synth

import stoi_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stoi_dev(eng, pairs, pad_e=0, pad_t=0, rate=10000):
    """pairs scored in one call, the estimates' buffer starting with pad_e spare samples and the targets' with pad_t ->
    (records [n, 8] numpy, one [segments, 2] array per clip)"""
    es, ts = [np.zeros(pad_e, np.float32)] + [p[0] for p in pairs], [np.zeros(pad_t, np.float32)] + [p[1] for p in pairs]
    eo, to = np.cumsum([0] + [len(x) for x in es]).tolist()[1:], np.cumsum([0] + [len(x) for x in ts]).tolist()[1:]
    rec, seg, soff = eng.stoi_device(dev(np.concatenate(es)), eo, dev(np.concatenate(ts)), to, rate=rate, per_segment=True)
    rec, seg = rec.cpu().numpy(), seg.cpu().numpy()
    per = []
    for i in range(len(pairs)):
        s = int(rec[i, 3])
        assert soff[i] + s <= soff[i + 1] and np.isnan(seg[soff[i] + s:soff[i + 1]]).all()     # nothing past the clip's segments
        per.append(seg[soff[i]:soff[i] + s])
    return rec, per


def as_dict(rec, per=None):
    d = score.stoi_record(rec)
    if per is not None:
        d["per_segment"] = per
    return d


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_lengths_and_compaction_within_the_bar_and_bit_equal(eng):
    pairs = S.length_clips() + [S.compaction_clip(k) for k in S.COMPACTION] + [S.clipped_clip(), S.opposed_clip()]
    alone = [stoi_dev(eng, [p]) for p in pairs]
    worst = {}
    for (rec, per), (e, t) in zip(alone, pairs):
        assert (rec[0, 6:] == 0.0).all()
        for k, v in S.stoi_ratios(as_dict(rec[0], per[0]), e, t).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("stoi lengths and compaction: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst
    # what the clips were chosen for
    counts = [tuple(int(v) for v in a[0][0, 1:4]) for a in alone]
    nl = len(S.LENGTHS)
    assert counts[:nl] == [(0, 0, 0)] * 3 + [(1, 1, 0), (1, 1, 0), (2, 2, 0), (30, 30, 0), (31, 31, 1), (31, 31, 1), (32, 32, 2),
                                             (32, 32, 2), (53, 53, 23)]
    assert counts[nl:nl + 6] == [(61, 61, 31), (61, 60, 30), (61, 60, 30), (65, 32, 2), (61, 31, 1), (61, 30, 0)]
    for i in list(range(7)) + [nl + 5]:
        assert math.isnan(alone[i][0][0, 4]) and math.isnan(alone[i][0][0, 5])           # no segment: NaN, the counts filled in
    assert alone[-1][0][0, 4] < 0.0                                                         # opposite envelopes
    # all of them in one batch, every offset odd (estimates from element 1 on, targets from element 3 on)
    rec, per = stoi_dev(eng, pairs, pad_e=1, pad_t=3)
    assert same_bits(rec, np.concatenate([a[0] for a in alone]))
    assert all(same_bits(p, a[1][0]) for p, a in zip(per, alone))
    rec2, per2 = stoi_dev(eng, pairs, pad_e=1, pad_t=3)
    assert same_bits(rec, rec2) and all(same_bits(a, b) for a, b in zip(per, per2))
    # another neighbourhood and another alignment: the same records
    rec3, _ = stoi_dev(eng, pairs[::-1], pad_e=2, pad_t=0)
    assert same_bits(rec3[::-1], rec)


def test_identity_and_edges(eng):
    e, t = S.clip(7001, 40)
    rec, per = stoi_dev(eng, [(t, t), (e, np.zeros(7001, np.float32)), (e, t[:5000]), (e[:4500], t)], pad_e=1)
    r = S.stoi_ratios(as_dict(rec[0], per[0]), t, t)
    assert max(r.values()) <= 1.0 and abs(rec[0, 4] - 1.0) < 1e-9 and abs(rec[0, 5] - 1.0) < 1e-9
    d = score.stoi_record(rec[1])
    assert (d["n"], d["frames"], d["frames_kept"], d["segments"]) == (7001, 53, 0, 0) and math.isnan(d["stoi"]) and math.isnan(d["estoi"])
    for i, (a, b) in ((2, (e[:5000], t[:5000])), (3, (e[:4500], t[:4500]))):
        assert score.stoi_record(rec[i])["n"] == len(a)
        assert max(S.stoi_ratios(as_dict(rec[i], per[i]), a, b).values()) <= 1.0
        assert same_bits(rec[i], stoi_dev(eng, [(a, b)])[0][0])                # the prefix, and nothing of what follows it
    out = eng.stoi_device(dev(np.zeros(0, np.float32)), [0], dev(np.zeros(0, np.float32)), [0])
    assert out.shape == (0, hip.STOI_FIELDS)
    assert eng.stoi([], []) == []


# ---- the conversion (the restatement of tests/test_gpu_resample.py for L = 5, M = 8) -----------------
L_, M_, HALF_, J_ = 5, 8, 80, 33


def _taps():
    """scipy.signal.resample_poly's default design for up 5, down 8: firwin(2 half + 1, 1 / 8, window=("kaiser", 5.0)) times 5"""
    from scipy.signal import firwin
    return L_ * firwin(2 * HALF_ + 1, 1.0 / max(L_, M_), window=("kaiser", 5.0))


def _cpu32(x):
    """The float32 restatement of y[m] on the CPU: taps rounded to float32, one sequential float32 accumulation per
    output (multiply, round, add, round), taps in the kernel's order."""
    h = np.zeros(L_ * J_, np.float32)
    t = _taps().astype(np.float32)
    h[:len(t)] = t
    n = len(x)
    m = np.arange(score.stoi_out_count(n), dtype=np.int64)
    q, p = np.divmod(m * M_ + HALF_, L_)
    xp = np.concatenate([np.zeros(J_, np.float32), np.asarray(x, np.float32), np.zeros(J_ + HALF_ // L_ + 2, np.float32)])
    acc = np.zeros(len(m), np.float32)
    for j in range(J_):
        k = q - j
        xv = np.where((k >= 0) & (k < n), xp[np.clip(k, -J_, n + J_) + J_], np.float32(0))
        acc = (h[p + j * L_] * xv).astype(np.float32) + acc
    return acc


def _resample_dev(eng, clips, pad=0):
    off = np.cumsum([pad] + [len(c) for c in clips]).tolist()
    o10 = np.cumsum([0] + [score.stoi_out_count(len(c)) for c in clips]).tolist()
    x = dev(np.concatenate([np.zeros(pad, np.float32)] + clips))
    y = torch.empty(max(o10[-1], 1), dtype=torch.float32, device="cuda")
    hip.check(eng.lib.nhans_stoi_resample(eng.handle, hip.ptr(x), hip.i64_array(off), len(clips), hip.ptr(y), hip.i64_array(o10),
                                          eng._stream()))
    y = y.cpu().numpy()
    return [y[o10[i]:o10[i + 1]] for i in range(len(clips))]


def test_conversion_against_resample_poly(eng):
    from scipy.signal import resample_poly
    rng = np.random.default_rng(5)
    n = 3213
    tt = np.arange(n) / 16000.0
    sweep = (0.9 * np.sin(2 * np.pi * (50 * tt + 0.5 * (0.45 * 16000 / tt[-1]) * tt * tt))).astype(np.float32)
    clips = [(0.3 * rng.standard_normal(n)).astype(np.float32), np.zeros(0, np.float32), sweep, sweep[:1].copy(), sweep[:J_ - 1].copy(),
             sweep[:1031].copy()]
    refs = [resample_poly(c.astype(np.float64), L_, M_) if len(c) else np.zeros(0) for c in clips]
    got = _resample_dev(eng, clips, pad=1)
    for g, r, c in zip(got, refs, clips):
        assert g.dtype == np.float32 and len(g) == len(r) == score.stoi_out_count(len(c)) == eng.lib.nhans_stoi_out_count(len(c))
    err_hip = max(float(np.abs(g - r).max()) for g, r in zip(got, refs) if len(r))
    err_cpu = max(float(np.abs(_cpu32(c) - r).max()) for c, r in zip(clips, refs) if len(r))
    peak = max(float(np.abs(r).max()) for r in refs if len(r))
    print("stoi resample 16000 -> 10000: err_hip %.3e  err_cpu32 %.3e  peak %.4e" % (err_hip, err_cpu, peak))
    assert err_hip <= 1.5 * err_cpu + 1e-7 * peak
    # stoi(rate=16000) is stoi(rate=10000) of the converted signals, bit for bit
    e16, t16 = S.clip(11003, 50)
    pairs16 = [(e16, t16), (e16[:7000], t16[:6900])]
    a = eng.stoi([p[0] for p in pairs16], [p[1] for p in pairs16], per_segment=True)
    conv = _resample_dev(eng, [x for p in pairs16 for x in p])
    b = eng.stoi(conv[0::2], conv[1::2], rate=10000, per_segment=True)
    for x, y in zip(a, b):
        assert x["segments"] >= 1 and {k: x[k] for k in score.STOI_FIELDS[:4]} == {k: y[k] for k in score.STOI_FIELDS[:4]}
        assert same_bits([x["stoi"], x["estoi"]], [y["stoi"], y["estoi"]]) and same_bits(x["per_segment"], y["per_segment"])
    rec, _ = stoi_dev(eng, list(zip(conv[0::2], conv[1::2])))
    assert same_bits(rec[:, 4:6], [[x["stoi"], x["estoi"]] for x in a])
    with pytest.raises(ValueError, match="16000 or 10000"):
        eng.stoi([e16], [t16], rate=8000)


def test_fixture_of_the_reference_demo_triples(eng):
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    worst = {}
    for ex in ("example2", "example3"):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        got = eng.stoi([sig["denoised"], sig["mixed"], sig["target"]], [sig["target"]] * 3)
        den, mix, same = got
        assert den["stoi"] > mix["stoi"] and den["estoi"] > mix["estoi"], (ex, den, mix)
        # held to the definition on the device's own converted signals
        conv = _resample_dev(eng, [sig["denoised"], sig["mixed"], sig["target"]])
        for rec, x in zip(got, conv):
            for k, v in S.stoi_ratios(rec, x, conv[2]).items():
                worst[k] = max(worst.get(k, 0.0), v)
        _, bar, _ = S.stoi_bar(conv[2], conv[2])
        assert abs(same["stoi"] - 1.0) <= bar["stoi"] + 4 * S.U and abs(same["estoi"] - 1.0) <= bar["estoi"] + 4 * S.U
        imp = score.improvement(mix, den)
        assert imp["stoi_i"] > 0 and imp["estoi_i"] > 0 and set(imp) == {"stoi_i", "estoi_i"}
        print("stoi fixture %s: mixed %.4f / %.4f  denoised %.4f / %.4f" % (ex, mix["stoi"], mix["estoi"], den["stoi"], den["estoi"]))
    print("stoi fixture: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


# ---- the surface -----------------------------------------------------------------------------------
def test_score_with_stoi_is_score_plus_stoi(eng):
    pairs = [S.clip(n, 80 + i) for i, n in enumerate((400, 7003, 11003))]
    es, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    plain, st, both = eng.score(es, ts), eng.stoi(es, ts), eng.score(es, ts, stoi=True)
    assert set(plain[0]) == set(score.FIELDS) | set(score.ROW_FIELDS)                      # today's keys
    for p, s, b in zip(plain, st, both):
        want = score.merge_stoi(p, s)
        assert set(b) == set(want) == set(p) | {"stoi_n", "stoi_frames", "frames_kept", "segments", "stoi", "estoi"}
        assert all(float(b[k]).hex() == float(want[k]).hex() for k in want)
    assert math.isnan(both[0]["stoi"]) and both[2]["segments"] >= 1 and both[2]["stoi_n"] == score.stoi_out_count(11003)
    assert eng.score([], [], stoi=True) == []


def _write_triple(tmp_path, tag, i, samples):
    from scipy.io import wavfile
    paths = []
    for name, x in (("speech", synth.mixture(30 + i, 2.6)[:samples]), ("pos", synth.noise_context(30 + i, 1.0)),
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


def test_evaluate_utterance_and_corpus_with_stoi(eng, tmp_path, monkeypatch):
    """Two triples whose network output is 7,000 and 7,500 samples long (one and three segments at 10 kHz) x two SNR pairs:
    the corpus pass equals the per-job call bit for bit, and the files are those written without the figures."""
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        triples = [_write_triple(tmp_path, "c", i, 32400 + 160 * extra) for i, extra in enumerate((44, 47))]
        pairs = [(-3, 5), (8, 0)]
        res = apply.evaluate_corpus(triples, snrs=pairs, stoi=True)
        plain = apply.evaluate_corpus(triples, snrs=pairs)
        assert len(res) == 4
        j = 0
        for triple in triples:
            for pair in pairs:
                with monkeypatch.context() as mp:
                    mp.setattr(mixing, "eval_snrs", lambda path: pair)
                    loss0 = apply.evaluate_utterance(*triple, str(tmp_path / "plain"), "nhans", 9)
                    loss, sc = apply.evaluate_utterance(*triple, str(tmp_path / "stoi"), "nhans", 9, scores=True, stoi=True)
                assert loss == loss0
                for name in ("denoised", "mixed"):
                    assert set(res[j][name]) == set(sc[name]) == set(plain[j][name]) | {"stoi_n", "stoi_frames", "frames_kept", "segments",
                                                                                       "stoi", "estoi"}
                    assert all(float(res[j][name][k]).hex() == float(sc[name][k]).hex() for k in sc[name]), (j, name)
                    assert all(float(res[j][name][k]).hex() == float(plain[j][name][k]).hex() for k in plain[j][name])
                    assert res[j][name]["segments"] >= 1 and math.isfinite(res[j][name]["stoi"]) and math.isfinite(res[j][name]["estoi"])
                assert set(res[j]["improvement"]) == set(plain[j]["improvement"]) | {"stoi_i", "estoi_i"} == set(sc["improvement"])
                assert res[j]["improvement"]["stoi_i"] == res[j]["denoised"]["stoi"] - res[j]["mixed"]["stoi"]
                j += 1
        assert len(_same_files(str(tmp_path / "plain"), str(tmp_path / "stoi"))) == 20
    finally:
        apply._engines.pop("denoiser", None)


def test_cli_with_stoi_leaves_the_audio_alone(eng, tmp_path, capsys):
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
        apply.main(["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav"), "--output", str(tmp_path / "plain.wav")] + common)
        capsys.readouterr()
        apply.main(["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav"), "--output", str(tmp_path / "scored.wav"),
                    "--score_against", str(tgd / "a.wav"), "--stoi"] + common)
        text = capsys.readouterr().out
        res = json.loads(text[text.index("{"):])
        (path, rec), = res["files"].items()
        for k in ("denoised", "mixed"):
            assert {"stoi", "estoi", "segments", "frames_kept", "stoi_n", "stoi_frames"} <= set(rec[k])
            assert rec[k]["segments"] >= 1 and -1.0 <= rec[k]["stoi"] <= 1.0 + 1e-9 and -1.0 <= rec[k]["estoi"] <= 1.0 + 1e-9
        assert rec["improvement"]["stoi_i"] == rec["denoised"]["stoi"] - rec["mixed"]["stoi"]
        for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
            assert open(str(tmp_path / ("plain" + tail)), "rb").read() == open(str(tmp_path / ("scored" + tail)), "rb").read()
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "o1")] + common)
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "o2"), "--score_against", str(tgd),
                    "--score_out", str(tmp_path / "s.json"), "--stoi"] + common)
        res = json.load(open(str(tmp_path / "s.json")))
        assert sorted(res["files"]) == [str(ind / "a.wav"), str(ind / "b.wav")]
        assert all(math.isfinite(f[k][fig]) for f in res["files"].values() for k in ("denoised", "mixed") for fig in ("stoi", "estoi"))
        assert res["mean"]["denoised"]["stoi"] == pytest.approx(np.mean([f["denoised"]["stoi"] for f in res["files"].values()]), rel=1e-15)
        assert "stoi_i" in res["mean"]["improvement"]
        _same_files(str(tmp_path / "o1"), str(tmp_path / "o2"))
    finally:
        apply._engines.pop("denoiser", None)
        for k in ("score_against", "score_out"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.stoi = False
        apply.FLAGS.input, apply.FLAGS.output, apply.FLAGS.neg, apply.FLAGS.pos = (apply.Flags.input, apply.Flags.output,
                                                                                    apply.Flags.neg, apply.Flags.pos)
        apply.FLAGS.weights = apply.Flags.weights
