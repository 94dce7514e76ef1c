"""LLR, cepstral distance and fwSegSNR on the device (quality.hip: nhans_quality) against the float64 definition
nhans_amd.score.quality_reference on identical input, within the bars of tests/quality_checks.py; the per-frame LPC
quantities bit for bit in the order the header states; records and per-frame values independent of batch, offset, order
and run; the select's rounding and ties; skipped frames; custom band matrices; the refusals; the input / output contract;
Context.score(quality=True); the fixture of the reference's own demo pairs; the command line.  Every test prints its
worst ratio to the bar (pytest -s)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import nhans_amd  # noqa: F401
from nhans_amd import apply, engine, hip, score, synth

import memory_checks as MC
import quality_checks as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


@pytest.fixture(scope="module")
def base():
    """the pair every size of Q.SIZES is a prefix of, with its reference, its bars and the header's order on the host"""
    e, t = Q.base_clip()
    ref, bars = Q.reference_with_bars(e, t)
    return e, t, ref, bars, Q.device_order_lpc(e, t)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buffers(clips, pads):
    ten, offs = [], []
    for k in (0, 1):
        xs = [np.full(pads[k], 1e30, np.float32)] + [c[k] for c in clips]
        offs.append(np.cumsum([0] + [len(x) for x in xs]).tolist()[1:])
        ten.append(dev(np.concatenate(xs)))
    return ten, offs


def quality_dev(eng, clips, pads=(0, 0), bands=None):
    """clips [(estimate, target)] scored in one call, either buffer starting with pads[k] spare samples (of a value that
    would show in every sum) -> (records [n, 16] numpy, [per-frame values [M_i, 3]])"""
    ten, offs = _buffers(clips, pads)
    rec, fr, foff = eng.quality_device(ten[0], offs[0], ten[1], offs[1], per_frame=True, bands=bands)
    fr = fr.cpu().numpy()
    return rec.cpu().numpy(), [fr[foff[i]:foff[i + 1]] for i in range(len(clips))]


def lpc_dev(eng, clips, pads=(0, 0)):
    """-> [rows of nhans_quality_lpc [M_i, 72]]"""
    ten, offs = _buffers(clips, pads)
    foff = np.cumsum([0] + [score.quality_num_frames(min(len(e), len(t))) for e, t in clips]).tolist()
    out = torch.empty((max(foff[-1], 1), hip.QUALITY_LPC_FIELDS), dtype=torch.float64, device="cuda")
    hip.check(eng.lib.nhans_quality_lpc(eng.handle, hip.ptr(ten[0]), hip.i64_array(offs[0]), hip.ptr(ten[1]), hip.i64_array(offs[1]),
                                        len(clips), hip.ptr(out), eng._stream()))
    out = out.cpu().numpy()
    return [out[foff[i]:foff[i + 1]] for i in range(len(clips))]


def worse(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), float(v))


def same_records(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y), (sorted(x), sorted(y))
        for k in x:
            if k == "per_frame":
                assert Q.same_bits(x[k], y[k])
            else:
                assert float(x[k]).hex() == float(y[k]).hex() or (math.isnan(x[k]) and math.isnan(y[k])), (k, x[k], y[k])


def everywhere_the_same(eng, clips, rec, per, rows, bands=None):
    """alone at aligned offsets, in the batch reversed at other offsets, and twice: the same bits"""
    for i, c in enumerate(clips):
        r1, p1 = quality_dev(eng, [c], bands=bands)
        assert Q.same_bits(r1[0], rec[i]) and Q.same_bits(p1[0], per[i]), i
    r2, p2 = quality_dev(eng, clips[::-1], pads=(2, 5), bands=bands)
    assert Q.same_bits(r2[::-1], rec) and all(Q.same_bits(a, b) for a, b in zip(p2[::-1], per))
    r3, p3 = quality_dev(eng, clips, pads=(1, 3), bands=bands)
    assert Q.same_bits(r3, rec) and all(Q.same_bits(a, b) for a, b in zip(p3, per))
    if rows is not None:
        rows2 = lpc_dev(eng, clips[::-1], pads=(4, 1))[::-1]
        assert all(Q.same_bits(a, b) for a, b in zip(rows2, rows))


def test_every_size_within_the_bars_and_bit_equal(eng, base):
    """n = 0, 479, 480, 599, 600, 601, one sample either side of every tile edge of the LPC launch and of the band launch, Mk =
    1, 10, 11, 30: all prefixes of one pair, scored in one batch at odd offsets."""
    e, t, ref, bars, order = base
    clips = [(e[:n], t[:n]) for n in Q.SIZES]
    rec, per = quality_dev(eng, clips, pads=(1, 3))
    rows = lpc_dev(eng, clips, pads=(1, 3))
    worst = {}
    assert (rec[:, 9:] == 0.0).all() and not np.signbit(rec[:, 9:]).any()
    for i, n in enumerate(Q.SIZES):
        M = score.quality_num_frames(n)
        got = score.quality_record(rec[i])
        assert (got["n"], got["frames"], len(per[i]), len(rows[i])) == (n, M, M, M)
        # the header's operation list, repeated on the host: the same bits
        assert Q.same_bits(rows[i], order[:M]), n
        if M == 0:
            assert got["frames_lpc"] == got["frames_fw"] == 0 and all(math.isnan(got[k]) for k in score.QUALITY_FIGURES), n
            continue
        r, b = Q.prefix(ref, bars, n)
        worse(worst, Q.quality_ratios(got, per[i], r, b, rows[i]))
    assert [score.quality_record(rec[Q.SIZES.index(Q.frames_to_samples(m))])["frames_lpc"] for m in (1, 10, 11, 30)] == [1, 10, 11, 30]
    everywhere_the_same(eng, clips, rec, per, rows)
    print("quality sizes %s: worst ratio to the bar" % (Q.SIZES,), json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


def test_three_seconds(eng):
    e, t = Q.clip(Q.LONG, 12)
    ref, bars = Q.reference_with_bars(e, t)
    rec, per = quality_dev(eng, [(e, t)], pads=(3, 1))
    rows = lpc_dev(eng, [(e, t)], pads=(3, 1))
    M = ref["frames"]
    frames = sorted(set(range(0, 9)) | set(range(195, 204)) | set(range(M - 9, M)))
    order = Q.device_order_lpc(e, t, frames=frames)
    assert M == 397 and Q.same_bits(rows[0][frames], order[frames])
    worst = Q.quality_ratios(score.quality_record(rec[0]), per[0], ref, bars, rows[0])
    short = (e[:5000], t[:4000])
    r2, p2 = quality_dev(eng, [short])
    everywhere_the_same(eng, [(e, t), short], np.stack([rec[0], r2[0]]), [per[0], p2[0]], None)
    print("quality 3 s (%d frames): worst ratio to the bar" % M, json.dumps({k: float(v) for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


def test_ties_skipped_frames_and_equal_signals(eng):
    """A clip whose frames repeat exactly (every value tied at the select's threshold); runs of zeros in the target
    (leading), the estimate (inner) and both (trailing); e == t."""
    pe, pt = Q.periodic_clip()
    ze, zt = Q.zero_runs_clip()
    be, bt = Q.base_clip()
    clips = [(pe, pt), (ze, zt), (bt[:2000], bt[:2000]), (np.zeros(1000, np.float32), np.zeros(1000, np.float32))]
    rec, per = quality_dev(eng, clips, pads=(3, 2))
    rows = lpc_dev(eng, clips, pads=(3, 2))
    worst = {}
    for i in (0, 1, 2):
        ref, bars = Q.reference_with_bars(*clips[i])
        worse(worst, Q.quality_ratios(score.quality_record(rec[i]), per[i], ref, bars, rows[i]))
        assert Q.same_values(rows[i], Q.device_order_lpc(*clips[i])), i
    # period 120: every frame has the bits of the first, and the trimmed mean of equal values is the value
    g = score.quality_record(rec[0])
    assert all(Q.same_bits(per[0][f], per[0][0]) for f in range(len(per[0]))) and g["frames_lpc"] == len(per[0]) == 11
    assert g["llr_95"] == per[0][0, 0] and g["cd_95_db"] == per[0][0, 1]
    # zeros: the frames inside a run are skipped and counted out
    z = score.quality_record(rec[1])
    sk = np.isnan(per[1])
    assert sk[:4].all() and sk[-4:].all() and sk[17:21, 0].all() and (np.abs(per[1][17:21, 2]) <= 35 * (score.QUALITY_BANDS + 4) * Q.U).all()
    assert z["frames"] == 47 and z["frames_lpc"] == int((~sk[:, 0]).sum()) < z["frames_fw"] == int((~sk[:, 2]).sum()) < 47
    # e == t: exactly 0, 0 and 35
    s = score.quality_record(rec[2])
    assert (s["llr"], s["llr_95"], s["cd_db"], s["cd_95_db"], s["fwsegsnr_db"]) == (0.0, 0.0, 0.0, 0.0, 35.0)
    assert (per[2][:, :2] == 0.0).all() and not np.signbit(per[2]).any() and (per[2][:, 2] == 35.0).all()
    # silence against silence: nothing kept, NaN, the counts filled in
    n = score.quality_record(rec[3])
    assert (n["n"], n["frames"], n["frames_lpc"], n["frames_fw"]) == (1000, 5, 0, 0) and all(math.isnan(n[k]) for k in score.QUALITY_FIGURES)
    everywhere_the_same(eng, clips, rec, per, None)
    print("quality ties, zero runs, e == t: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("K", [1, 32])
def test_custom_band_matrix(eng, K):
    W = Q.custom_bands(K)
    e, t = Q.base_clip()
    clips = [(e[:1321], t[:1321]), (e[600:1800], t[600:1800])]
    rec, per = quality_dev(eng, clips, pads=(1, 1), bands=W)
    worst = {}
    for i, c in enumerate(clips):
        ref, bars = Q.reference_with_bars(*c, bands=W)
        worse(worst, Q.quality_ratios(score.quality_record(rec[i]), per[i], ref, bars))
    plain, _ = quality_dev(eng, clips, pads=(1, 1))
    assert Q.same_bits(plain[:, :8], rec[:, :8]) and not Q.same_bits(plain[:, 8], rec[:, 8])        # the bands move fwSegSNR alone
    everywhere_the_same(eng, clips, rec, per, None, bands=W)
    print("quality custom bands K %d: worst ratio to the bar" % K, json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


def test_default_bands_passed_explicitly_change_nothing(eng):
    e, t = Q.base_clip()
    a, pa = quality_dev(eng, [(e[:2000], t[:2000])])
    b, pb = quality_dev(eng, [(e[:2000], t[:2000])], bands=score.quality_band_matrix())
    assert Q.same_bits(a, b) and Q.same_bits(pa[0], pb[0])


def test_refusals_name_the_clip_and_touch_nothing(eng):
    x = np.arange(1200, dtype=np.float32)
    src = MC.Surrounded("f32", [x], [0], size=1200, device=eng.device)
    before = src.host_bits().copy()
    outs = [MC.Guarded("f64", 512, which=w, device=eng.device) for w in (0, 1)]
    for g in outs:
        Q.check_refusals(eng.lib, eng.handle, buf=ctypes.c_void_p(src.ptr), out=ctypes.c_void_p(g.ptr))
    torch.cuda.synchronize()
    f = MC.findings(outs, np.zeros(512, bool))
    assert not f, MC.report(f)
    assert np.array_equal(src.host_bits(), before)
    with pytest.raises(ValueError, match="one target per estimate"):
        eng.quality([x], [])
    with pytest.raises(ValueError, match="257"):
        eng.quality([x], [x], bands=np.ones((2, 256)))
    assert eng.quality([], []) == []
    out = eng.quality_device(dev(np.zeros(0, np.float32)), [0], dev(np.zeros(0, np.float32)), [0])
    assert out.shape == (0, hip.QUALITY_FIELDS)


def test_contract_of_nhans_quality(eng):
    """The call writes its documented elements and nothing beside them, and reads no sample outside the clips: three runs --
    exact sizes; guarded outputs and inputs surrounded by zeros; the other sentinel and inputs surrounded by NaN -- give
    the same bits."""
    e, t = Q.base_clip()
    pairs = [(e[:0], t[:4]), (e[:479], t[:600]), (e[:1321], t[:1300]), (e[100:1000], t[100:1000])]
    sig = [[p[0] for p in pairs], [p[1] for p in pairs]]
    n = len(pairs)
    M = sum(score.quality_num_frames(min(len(a), len(b))) for a, b in pairs)
    p = lambda b: ctypes.c_void_p(b.ptr)
    runs = {}
    for layout in ("exact", "A", "B"):
        guarded = layout != "exact"
        ins = []
        for k in (0, 1):
            off = MC.tight_offsets([len(x) for x in sig[k]])
            ins.append((MC.Surrounded("f32", sig[k], off[:-1], size=off[-1], align=(1 + k) % 4 if guarded else 0,
                                      variant="B" if layout == "B" else "A", device=eng.device), off))
        outs = [MC.Guarded("f64", size + (3 if guarded else 0), align=int(guarded), which=int(layout == "B"), device=eng.device)
                for size in (n * hip.QUALITY_FIELDS, 3 * M, hip.QUALITY_LPC_FIELDS * M)]
        rc = eng.lib.nhans_quality(eng.handle, p(ins[0][0]), hip.i64_array(ins[0][1]), p(ins[1][0]), hip.i64_array(ins[1][1]), n,
                                   None, 0, p(outs[0]), p(outs[1]), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        rc = eng.lib.nhans_quality_lpc(eng.handle, p(ins[0][0]), hip.i64_array(ins[0][1]), p(ins[1][0]), hip.i64_array(ins[1][1]), n,
                                       p(outs[2]), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        torch.cuda.synchronize()
        runs[layout] = outs
    for k, size in enumerate((n * hip.QUALITY_FIELDS, 3 * M, hip.QUALITY_LPC_FIELDS * M)):
        mask = np.concatenate([np.ones(size, bool), np.zeros(3, bool)])
        f = MC.findings([runs["A"][k], runs["B"][k]], mask)
        assert not f, MC.report(f)
        ex, a, b = (runs[layout][k].region_bits()[:size] for layout in ("exact", "A", "B"))
        assert np.array_equal(a, ex) and np.array_equal(b, a), k
    rec = runs["exact"][0].region().reshape(n, hip.QUALITY_FIELDS)
    assert rec[:, 0].tolist() == [0, 479, 1300, 900] and rec[:, 1].tolist() == [0, 0, 7, 4] and M == 11
    # without frames_out the records are the same
    plain = eng.quality_device(dev(np.concatenate(sig[0])), MC.tight_offsets([len(x) for x in sig[0]]), dev(np.concatenate(sig[1])),
                               MC.tight_offsets([len(x) for x in sig[1]])).cpu().numpy()
    assert Q.same_bits(plain, rec)


# ---- the surface -----------------------------------------------------------------------------------
def test_score_with_quality_equals_the_separate_call(eng):
    e, t = Q.base_clip()
    es, ts = [e[:3003], e[500:2500], e[:400]], [t[:3000], t[500:2700], t[:400]]
    plain = eng.score(es, ts)
    assert set(plain[0]) == set(score.FIELDS) | set(score.ROW_FIELDS)          # today's keys without the flag
    q = eng.quality(es, ts, per_frame=True)
    assert set(q[0]) == set(score.QUALITY_FIELDS) | {"per_frame"} and [r["frames"] for r in q] == [22, 13, 0]
    got = eng.score(es, ts, quality=True)
    same_records(got, [score.merge_quality(p, {k: v for k, v in r.items() if k != "per_frame"}) for p, r in zip(plain, q)])
    assert got[0]["n"] == 3000 and got[0]["quality_n"] == 3000 and got[0]["quality_frames"] == 22 and "llr" in got[0]
    same_records([{k: r[k] for k in plain[0]} for r in got], plain)               # records without the flag: unchanged
    both = eng.score(es, ts, quality=True, stoi=True, bss=True)
    assert set(both[0]) >= set(got[0]) | {"stoi", "sdr_db"}
    same_records([{k: r[k] for k in got[0]} for r in both], got)
    # delays: through the same cut pairs
    cut = [score.align_cut(a, b, d) for a, b, d in zip(es, ts, (5, -7, 0))]
    want = eng.score([c[0] for c in cut], [c[1] for c in cut], quality=True)
    same_records(eng.score(es, ts, quality=True, delays=[5, -7, 0]), [dict(w, delay=d) for w, d in zip(want, (5, -7, 0))])
    same_records(eng.quality(es, ts, delays=[5, -7, 0]), [dict(w, delay=d) for w, d in zip(eng.quality([c[0] for c in cut], [c[1] for c in cut]), (5, -7, 0))])
    imp = score.improvement(got[1], got[0])
    assert {"llr_i", "llr_95_i", "cd_i", "cd_95_i", "fwsegsnr_i"} <= set(imp) and imp["llr_i"] == got[0]["llr"] - got[1]["llr"]
    print("quality surface: score(quality=True) bit-equal to the separate call: worst ratio to the bar 0")


def test_fixture_of_the_reference_demo_pairs(eng):
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    worst = {}
    for ex in ("example2", "example3"):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        got = eng.quality([sig["denoised"], sig["mixed"]], [sig["target"], sig["target"]], per_frame=True)
        for name, r in zip(("denoised", "mixed"), got):
            ref, bars = Q.reference_with_bars(sig[name], sig["target"])
            worse(worst, Q.quality_ratios(r, r["per_frame"], ref, bars))
            print("quality fixture %s %s: frames %d lpc %d fw %d, llr %.4f llr_95 %.4f cd %.4f dB cd_95 %.4f dB fwsegsnr %.3f dB"
                  % (ex, name, r["frames"], r["frames_lpc"], r["frames_fw"], r["llr"], r["llr_95"], r["cd_db"], r["cd_95_db"], r["fwsegsnr_db"]))
        imp = score.improvement(got[1], got[0])
        print("quality fixture %s improvement: llr_i %.4f cd_i %.4f fwsegsnr_i %.3f" % (ex, imp["llr_i"], imp["cd_i"], imp["fwsegsnr_i"]))
    print("quality fixture: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


QUALITY_KEYS = {"quality_n", "quality_frames", "frames_lpc", "frames_fw"} | set(score.QUALITY_FIGURES)


def test_evaluate_utterance_and_corpus_with_quality(eng, tmp_path, monkeypatch):
    """One triple at one SNR pair: the corpus pass equals the per-job call bit for bit, without the flag both return what
    they returned before, and the files are those written without the figures."""
    from scipy.io import wavfile
    from nhans_amd import mixing
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        triple = []
        for name, x in (("speech", synth.mixture(51, 2.6)[:32400 + 160 * 44]), ("pos", synth.noise_context(51, 1.0)),
                        ("neg", synth.speaker_context(51, 3.0))):
            triple.append(str(tmp_path / ("q_%s.wav" % name)))
            wavfile.write(triple[-1], 16000, x)
        pair = (-3, 5)
        res = apply.evaluate_corpus([tuple(triple)], snrs=[pair], quality=True)
        plain = apply.evaluate_corpus([tuple(triple)], snrs=[pair])
        with monkeypatch.context() as mp:
            mp.setattr(mixing, "eval_snrs", lambda path: pair)
            loss0, sc0 = apply.evaluate_utterance(*triple, str(tmp_path / "plain"), "nhans", 9, scores=True)
            loss, sc = apply.evaluate_utterance(*triple, str(tmp_path / "quality"), "nhans", 9, scores=True, quality=True)
        assert loss == loss0 and len(res) == 1
        for name in ("denoised", "mixed"):
            assert set(res[0][name]) == set(sc[name]) == set(plain[0][name]) | QUALITY_KEYS
            assert set(sc0[name]) == set(plain[0][name]) == set(score.FIELDS) | set(score.ROW_FIELDS)           # today's keys
            assert all(float(res[0][name][k]).hex() == float(sc[name][k]).hex() for k in sc[name]), name
            assert all(float(res[0][name][k]).hex() == float(plain[0][name][k]).hex() for k in plain[0][name])
            assert all(float(sc0[name][k]).hex() == float(sc[name][k]).hex() for k in sc0[name])
            assert res[0][name]["frames_lpc"] > 0 and all(math.isfinite(res[0][name][k]) for k in score.QUALITY_FIGURES)
        new = {"llr_i", "llr_95_i", "cd_i", "cd_95_i", "fwsegsnr_i"}
        assert set(res[0]["improvement"]) == set(plain[0]["improvement"]) | new == set(sc["improvement"])
        assert set(sc0["improvement"]) == set(plain[0]["improvement"])
        assert res[0]["improvement"]["cd_i"] == res[0]["denoised"]["cd_db"] - res[0]["mixed"]["cd_db"]
        names = sorted(os.listdir(str(tmp_path / "plain")))
        assert names == sorted(os.listdir(str(tmp_path / "quality"))) and len(names) == 5
        for name in names:
            assert open(str(tmp_path / "plain" / name), "rb").read() == open(str(tmp_path / "quality" / name), "rb").read(), name
    finally:
        apply._engines.pop("denoiser", None)


# ---- the command line ------------------------------------------------------------------------------
def test_cli_with_quality(eng, tmp_path, capsys):
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        clean = synth.mixture(43, 1.0)
        noise = synth.noise_context(43, 1.0)
        mixed = (clean.astype(np.int32) // 2 + noise[:len(clean)].astype(np.int32) // 4).astype(np.int16)
        wavfile.write(str(tmp_path / "in.wav"), 16000, mixed)
        wavfile.write(str(tmp_path / "neg.wav"), 16000, noise)
        wavfile.write(str(tmp_path / "tgt.wav"), 16000, clean // 2)
        common = ["--input", str(tmp_path / "in.wav"), "--neg", str(tmp_path / "neg.wav"), "--pos", str(tmp_path / "Silent.wav"),
                  "--weights", "synthetic"]
        apply.main(common + ["--output", str(tmp_path / "plain.wav"), "--score_against", str(tmp_path / "tgt.wav")])
        text = capsys.readouterr().out
        plain = json.loads(text[text.index("{"):])
        apply.main(common + ["--output", str(tmp_path / "scored.wav"), "--score_against", str(tmp_path / "tgt.wav"), "--quality"])
        text = capsys.readouterr().out
        res = json.loads(text[text.index("{"):])
        (_, rec), = res["files"].items()
        (_, old), = plain["files"].items()
        den, mix = apply.wavread(str(tmp_path / "scored.wav"))[1], apply.wavread(str(tmp_path / "scored_mixed_processed.wav"))[1]
        t = apply.scaled_target(str(tmp_path / "in.wav"), str(tmp_path / "tgt.wav"))
        hand = eng.quality([den, mix], [t, t])
        for k, h in zip(("denoised", "mixed"), hand):
            assert set(rec[k]) == set(old[k]) | {"quality_n", "quality_frames", "frames_lpc", "frames_fw"} | set(score.QUALITY_FIGURES)
            assert all(float(rec[k][f]).hex() == float(old[k][f]).hex() for f in old[k]), k           # without the flag: the same bits
            assert all(float(rec[k][f]).hex() == float(h[f]).hex() for f in score.QUALITY_FIGURES), k
            assert rec[k]["frames_lpc"] > 0
        assert {"llr_i", "cd_i", "fwsegsnr_i"} <= set(rec["improvement"]) and not {"llr_i"} & set(old["improvement"])
        for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
            assert open(str(tmp_path / ("plain" + tail)), "rb").read() == open(str(tmp_path / ("scored" + tail)), "rb").read()
        with pytest.raises(SystemExit):
            apply.main(common + ["--output", str(tmp_path / "x.wav"), "--quality"])
        print("quality cli: llr mixed %.4f denoised %.4f, fwsegsnr mixed %.3f denoised %.3f: figures bit-equal to the separate call's: worst ratio to the bar 0"
              % (rec["mixed"]["llr"], rec["denoised"]["llr"], rec["mixed"]["fwsegsnr_db"], rec["denoised"]["fwsegsnr_db"]))
    finally:
        apply._engines.pop("denoiser", None)
        for k in ("score_against", "score_out"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.quality = False
        apply.FLAGS.input, apply.FLAGS.output, apply.FLAGS.neg, apply.FLAGS.pos = (apply.Flags.input, apply.Flags.output,
                                                                                    apply.Flags.neg, apply.Flags.pos)
        apply.FLAGS.weights = apply.Flags.weights
