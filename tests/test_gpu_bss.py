"""BSS Eval on the device (bsseval.hip, nhans_bss_eval) against the float64 definition nhans_amd.score.bss_reference on
identical input, within the bar of tests/bss_checks.py; the coefficients against the normal equations; the records'
independence of batch, offset, run and group, bit for bit; the edges; the refusals; the fixture of the reference's own demo
triples; Context.score(bss=...), evaluate_utterance, evaluate_corpus and the command line; the input / output contract of
the call.  Every test prints its worst ratio to the bar (pytest -s)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import nhans_amd  # noqa: F401
from nhans_amd import apply, context, engine, hip, mixing, score, synth

import bss_checks as B
import memory_checks as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bss_dev(eng, clips, L, pads=(0, 0, 0), filters=True):
    """clips [(estimate, sources)] (all with as many sources) scored in one call, signal k's buffer starting with pads[k]
    spare samples -> (records [n, 16] numpy, filters [n, (J + 1) L] numpy)"""
    J = len(clips[0][1])
    sigs = [[c[0] for c in clips]] + [[c[1][j] for c in clips] for j in range(J)]
    ten, offs = [], []
    for k, xs in enumerate(sigs):
        xs = [np.zeros(pads[k], np.float32)] + list(xs)
        offs.append(np.cumsum([0] + [len(x) for x in xs]).tolist()[1:])
        ten.append(dev(np.concatenate(xs)))
    rec, filt = eng.bss_eval_device(ten[0], offs[0], list(zip(ten[1:], offs[1:])), filt_len=L, filters=True)
    return rec.cpu().numpy(), filt.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def worse(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def normal_ratios(filt, ref, bar, L):
    """the device's coefficients in the reference's normal equations: |G C - D|_2 and |G_00 C0 - D[:L]|_2 over their bars"""
    M = ref["J"] * L
    C, C0 = filt[:M], filt[M:]
    return {"normal": float(np.linalg.norm(ref["G"] @ C - ref["D"])) / bar["normal"],
            "normal0": float(np.linalg.norm(ref["G"][:L, :L] @ C0 - ref["D"][:L])) / bar["normal0"]}


@pytest.mark.parametrize("L,J", sorted({(s[0], s[1]) for s in B.SHAPES}))
def test_every_shape_within_the_bar_and_bit_equal(eng, L, J):
    worst = {}
    shapes = [s for s in B.SHAPES if (s[0], s[1]) == (L, J)]
    clips = [B.shape_clip(s) for s in shapes]
    rec, filt = bss_dev(eng, clips, L, pads=(1, 3, 2))
    assert (rec[:, 13:] == 0.0).all()
    for i, (s, (e, src)) in enumerate(zip(shapes, clips)):
        ref, bar = B.bss_bar(e, src, L)
        worse(worst, B.bss_ratios(score.bss_record(rec[i]), e, src, L, may_drop=B.may_drop(s), ref=ref))
        worse(worst, normal_ratios(filt[i], ref, bar, L))
        if J == 1:
            assert rec[i, 10] == math.inf and rec[i, 5] == 0.0 and rec[i, 11] == rec[i, 9]      # SIR, E_int; SAR has SDR's value
            assert same_bits(filt[i][:L], filt[i][L:])
        # alone, at aligned offsets: the same bits
        r1, f1 = bss_dev(eng, [clips[i]], L)
        assert same_bits(r1[0], rec[i]) and same_bits(f1[0], filt[i]), (s, r1[0], rec[i])
    rec2, filt2 = bss_dev(eng, clips, L, pads=(1, 3, 2))
    assert same_bits(rec, rec2) and same_bits(filt, filt2)
    # another neighbourhood and another alignment: the same records
    rec3, filt3 = bss_dev(eng, clips[::-1], L, pads=(2, 0, 1))
    assert same_bits(rec3[::-1], rec) and same_bits(filt3[::-1], filt)
    print("bss shapes L %d J %d (n %s): worst ratio to the bar" % (L, J, ", ".join(str(s[2]) for s in shapes)), json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


def test_rank_deficient_shapes(eng):
    """Two sources and fewer samples than unknowns: what can be asserted without a bar (tests/bss_checks.py)."""
    for L in sorted({s[0] for s in B.EDGE_SHAPES}):
        shapes = [s for s in B.EDGE_SHAPES if s[0] == L]
        clips = [B.shape_clip(s) for s in shapes]
        rec, filt = bss_dev(eng, clips, L, pads=(3, 1, 2))
        for i, s in enumerate(shapes):
            d = score.bss_record(rec[i])
            assert (d["n"], d["J"], d["L"]) == (s[2], 2, L) and d["singular"] in (0, 1)
            if d["singular"]:
                assert np.isnan(rec[i, 3:12]).all() and np.isnan(filt[i]).all()
            r1, f1 = bss_dev(eng, [clips[i]], L)
            assert same_bits(r1[0], rec[i]) and same_bits(f1[0], filt[i])


def test_group_boundary_changes_no_bit(eng):
    """Eight clips of L = 16, J = 2 (a factor of 8 KiB each) in groups of three, of one and in one group."""
    L = 16
    clips = [B.clip(n, a, 700 + i) for i, (n, a) in enumerate(((2049, 0.9), (300, 0.5), (4000, 0.99), (0, 0.5), (1024, 0.9), (2048, 0.5),
                                                                (77, 0.5), (1500, 0.9)))]
    clips[6] = (clips[6][0], [clips[6][1][0], np.zeros(77, np.float32)])           # a singular clip inside a group
    whole = bss_dev(eng, clips, L, pads=(1, 2, 3))
    assert whole[0][3, 12] == 1.0 and whole[0][6, 12] == 1.0 and (whole[0][[0, 1, 2, 4, 5, 7], 12] == 0.0).all()
    try:
        for bound in (3 * 8 * (2 * L) ** 2, 1):
            eng.set_option("bss_group_bytes", bound)
            got = bss_dev(eng, clips, L, pads=(1, 2, 3))
            assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]), bound
    finally:
        eng.set_option("bss_group_bytes", 2 << 30)
    with pytest.raises(hip.NhansError, match="bss_group_bytes"):
        eng.set_option("bss_group_bytes", 0)


def test_edges(eng):
    L = 16
    e, (s0, s1) = B.clip(3000, 0.9, 720)
    zero = np.zeros(3000, np.float32)
    clips = [(e[:0], [s0, s1]), (e, [s0, zero]), (s0.copy(), [s0, s1]), (e, [s0[:2500], s1]), (np.concatenate([e[:2500], np.ones(9, np.float32)]), [s0, s1[:2500]])]
    rec, filt = bss_dev(eng, clips, L, pads=(1, 0, 2))
    # no samples: NaN
    d = score.bss_record(rec[0])
    assert (d["n"], d["J"], d["L"], d["singular"]) == (0, 2, L, 1) and np.isnan(rec[0, 3:12]).all()
    # an all-zero interferer: singular, NaN figures, the counts filled in
    d = score.bss_record(rec[1])
    assert (d["n"], d["J"], d["L"], d["singular"]) == (3000, 2, L, 1) and np.isnan(rec[1, 3:12]).all() and np.isnan(filt[1]).all()
    assert (rec[:2, 13:] == 0.0).all()
    r = B.bss_ratios(d, *clips[1], L)
    assert max(r.values()) == 0.0
    # the estimate bit-equal to s_0: E_dist at rounding level, compared as an energy
    ref, bar = B.bss_bar(*clips[2], L)
    d = score.bss_record(rec[2])
    assert d["singular"] == 0 and ref["E_dist"] <= 1e-24 * ref["E_e"]
    r = {k: B.ratio(d[k] / ref["E_e"], ref[k] / ref["E_e"], bar[k]) for k in score.BSS_ENERGIES}
    print("bss estimate == target: energies' worst ratio to the bar %.3g, E_dist / E_e %.3g" % (max(r.values()), d["E_dist"] / d["E_e"]))
    assert max(r.values()) <= 1.0, r
    assert abs(filt[2][0] - 1.0) < 1e-9 and np.abs(filt[2][2 * L + 1:]).max() < 1e-9                 # C0 = (1, 0, ...)
    # the common prefix, and nothing of what follows it
    for i in (3, 4):
        assert score.bss_record(rec[i])["n"] == 2500
        assert same_bits(rec[i], bss_dev(eng, [(e[:2500], [s0[:2500], s1[:2500]])], L)[0][0])
    out = eng.bss_eval_device(dev(np.zeros(0, np.float32)), [0], [(dev(np.zeros(0, np.float32)), [0])])
    assert out.shape == (0, hip.BSS_FIELDS)
    assert eng.bss_eval([], [], []) == []


def test_refusals_name_the_clip(eng):
    B.check_refusals(eng.lib, eng.handle)
    with pytest.raises(ValueError, match="one target and one interferer per estimate"):
        eng.bss_eval([np.zeros(4, np.float32)], [np.zeros(4, np.float32)], [])


def test_fixture_of_the_reference_demo_triples(eng):
    """The interferer is mixed - target; L = 128 keeps the float64 reference of the four records to seconds.  The mixture
    lies in the span of target and mixture - target: its SAR is the one figure the cap may drop."""
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    L, worst = 128, {}
    for ex in ("example2", "example3"):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        interf = (sig["mixed"] - sig["target"]).astype(np.float32)
        den, mix = eng.bss_eval([sig["denoised"], sig["mixed"]], [sig["target"]] * 2, [interf] * 2, filt_len=L)
        worse(worst, B.bss_ratios(den, sig["denoised"], [sig["target"], interf], L))
        worse(worst, B.bss_ratios(mix, sig["mixed"], [sig["target"], interf], L, may_drop=("sar_db",)))
        imp = score.improvement(mix, den)
        assert set(imp) == {"sdr_i", "sir_i", "sar_i"} and imp["sdr_i"] > 0 and imp["sir_i"] > 0, (ex, imp)
        assert abs(mix["sdr_db"] - mix["sir_db"]) < 1e-6 and mix["sar_db"] > 100.0               # no artifacts in the mixture
        print("bss fixture %s (L %d): mixed %.2f / %.2f  denoised %.2f / %.2f / %.2f" % (ex, L, mix["sdr_db"], mix["sir_db"], den["sdr_db"],
                                                                                          den["sir_db"], den["sar_db"]))
    print("bss fixture: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


# ---- the surface -----------------------------------------------------------------------------------
def test_score_with_bss_is_score_plus_bss_eval(eng):
    clips = [B.clip(n, 0.9, 740 + i) for i, n in enumerate((400, 3003, 5003))]
    es, ts, ns = [c[0] for c in clips], [c[1][0] for c in clips], [c[1][1] for c in clips]
    plain, bs, both = eng.score(es, ts), eng.bss_eval(es, ts, ns), eng.score(es, ts, bss=ns)
    assert set(plain[0]) == set(score.FIELDS) | set(score.ROW_FIELDS)                      # today's keys
    for p, b, m in zip(plain, bs, both):
        want = score.merge_bss(p, b)
        assert set(m) == set(want) == set(p) | {"bss_n"} | (set(score.BSS_FIELDS) - {"n"})
        assert all(float(m[k]).hex() == float(want[k]).hex() for k in want)
    assert both[2]["bss_n"] == 5003 and math.isfinite(both[2]["sir_db"]) and both[2]["L"] == 512
    one = eng.score(es, ts, bss=True)
    assert all(r["J"] == 1 and r["sir_db"] == math.inf for r in one)
    f = eng.bss_eval(es[:1], ts[:1], ns[:1], filt_len=8, filters=True)[0]
    assert f["C"].shape == (2, 8) and f["C0"].shape == (8,) and abs(f["C"][0, 0] - 0.8) < 0.1
    assert eng.score([], [], bss=[]) == []


# ---- the input / output contract (the helpers of tests/memory_checks.py) ---------------------------
def test_contract_of_nhans_bss_eval(eng):
    """The call writes the records and the filters and nothing beside them, and reads no sample outside the clips: three
    runs -- exact sizes; guarded outputs and inputs surrounded by zeros; the other sentinel and inputs surrounded by NaN --
    give the same bits."""
    L, J = 16, 2
    clips = [B.clip(n, 0.9, 760 + i) for i, n in enumerate((0, 1, 2049, 300))]
    est = [c[0] for c in clips]
    est[3] = np.concatenate([est[3], np.ones(11, np.float32)])                  # the common prefix counts
    srcs = [[c[1][j] for c in clips] for j in range(J)]
    n, sizes = len(clips), (len(clips) * hip.BSS_FIELDS, len(clips) * (J + 1) * L)
    runs = {}
    for layout in ("exact", "A", "B"):
        guarded = layout != "exact"
        ins = []
        for k, pieces in enumerate([est] + srcs):
            counts = [len(p) for p in pieces]
            off = MC.tight_offsets(counts)                                      # (the offsets ARE the clips: no slack between them)
            ins.append((MC.Surrounded("f32", pieces, off[:-1], size=off[-1], align=(1 + k) % 4 if guarded else 0,
                                      variant="B" if layout == "B" else "A", device=eng.device), off))
        outs = [MC.Guarded("f64", size + (3 if guarded else 0), align=int(guarded), which=int(layout == "B"), device=eng.device)
                for size in sizes]
        p = lambda b: ctypes.c_void_p(b.ptr)
        rc = context.bss_call(eng.lib, eng.handle, p(ins[0][0]), ins[0][1], [p(b) for b, _ in ins[1:]], [o for _, o in ins[1:]], n, L,
                              p(outs[0]), p(outs[1]), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        torch.cuda.synchronize()
        runs[layout] = outs
    for k, size in enumerate(sizes):
        mask = np.concatenate([np.ones(size, bool), np.zeros(3, bool)])
        f = MC.findings([runs["A"][k], runs["B"][k]], mask)
        assert not f, MC.report(f)
        ex, a, b = (runs[layout][k].region_bits()[:size] for layout in ("exact", "A", "B"))
        assert np.array_equal(a, ex) and np.array_equal(b, a), k
    rec = runs["exact"][0].region().reshape(n, hip.BSS_FIELDS)
    assert rec[:, 0].tolist() == [0, 1, 2049, 300] and rec[:, 12].tolist() == [1, 1, 0, 0]


# ---- evaluate_utterance, evaluate_corpus and the command line ---------------------------------------
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


BSS_KEYS = {"bss_n"} | (set(score.BSS_FIELDS) - {"n"})


def test_evaluate_utterance_and_corpus_with_bss(eng, tmp_path, monkeypatch):
    """Two triples x two SNR pairs: the corpus pass equals the per-job call bit for bit, without bss both return what they
    returned before, and the files are those written without the figures."""
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        triples = [_write_triple(tmp_path, "c", i, 32400 + 160 * extra) for i, extra in enumerate((44, 47))]
        pairs = [(-3, 5), (8, 0)]
        res = apply.evaluate_corpus(triples, snrs=pairs, bss=True)
        plain = apply.evaluate_corpus(triples, snrs=pairs)
        assert len(res) == 4
        j = 0
        for triple in triples:
            for pair in pairs:
                with monkeypatch.context() as mp:
                    mp.setattr(mixing, "eval_snrs", lambda path: pair)
                    loss0, sc0 = apply.evaluate_utterance(*triple, str(tmp_path / "plain"), "nhans", 9, scores=True)
                    loss, sc = apply.evaluate_utterance(*triple, str(tmp_path / "bss"), "nhans", 9, scores=True, bss=True)
                assert loss == loss0
                for name in ("denoised", "mixed"):
                    assert set(res[j][name]) == set(sc[name]) == set(plain[j][name]) | BSS_KEYS
                    assert set(sc0[name]) == set(plain[j][name]) == set(score.FIELDS) | set(score.ROW_FIELDS)       # today's keys
                    assert all(float(res[j][name][k]).hex() == float(sc[name][k]).hex() for k in sc[name]), (j, name)
                    assert all(float(res[j][name][k]).hex() == float(plain[j][name][k]).hex() for k in plain[j][name])
                    assert all(float(sc0[name][k]).hex() == float(sc[name][k]).hex() for k in sc0[name])
                    r = res[j][name]
                    assert (r["J"], r["L"], r["singular"], r["bss_n"]) == (2, 512, 0, r["n"]) and all(math.isfinite(r[k]) for k in score.BSS_FIGURES)
                assert set(res[j]["improvement"]) == set(plain[j]["improvement"]) | {"sdr_i", "sir_i", "sar_i"} == set(sc["improvement"])
                assert set(sc0["improvement"]) == set(plain[j]["improvement"])
                assert res[j]["improvement"]["sir_i"] == res[j]["denoised"]["sir_db"] - res[j]["mixed"]["sir_db"]
                j += 1
        assert len(_same_files(str(tmp_path / "plain"), str(tmp_path / "bss"))) == 20
    finally:
        apply._engines.pop("denoiser", None)


def test_cli_with_bss_leaves_the_audio_alone(eng, tmp_path, capsys):
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        clean = synth.mixture(41, 1.0)
        noise = synth.noise_context(41, 1.0)
        mixed = (clean.astype(np.int32) // 2 + noise[:len(clean)].astype(np.int32) // 4).astype(np.int16)
        ind, tgd, negd, ifd = tmp_path / "in", tmp_path / "tgt", tmp_path / "neg", tmp_path / "interf"
        for d in (ind, tgd, negd, ifd):
            d.mkdir()
        for name, k in (("a.wav", len(mixed)), ("b.wav", len(mixed) - 1000)):
            wavfile.write(str(ind / name), 16000, mixed[:k])
            wavfile.write(str(tgd / name), 16000, (clean // 2)[:k])
            wavfile.write(str(ifd / name), 16000, (noise[:len(clean)] // 4)[:k])
            wavfile.write(str(negd / name), 16000, noise)
        common = ["--pos", str(tmp_path / "Silent.wav"), "--weights", "synthetic"]
        apply.main(["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav"), "--output", str(tmp_path / "plain.wav")] + common)
        capsys.readouterr()
        apply.main(["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav"), "--output", str(tmp_path / "scored.wav"),
                    "--score_against", str(tgd / "a.wav"), "--bss", "--interferer", str(ifd / "a.wav")] + common)
        text = capsys.readouterr().out
        res = json.loads(text[text.index("{"):])
        (path, rec), = res["files"].items()
        for k in ("denoised", "mixed"):
            assert BSS_KEYS <= set(rec[k]) and rec[k]["singular"] == 0 and rec[k]["J"] == 2 and rec[k]["L"] == 512
            assert all(math.isfinite(rec[k][f]) for f in ("sdr_db", "sir_db"))
        # the mixed round trip is target + interferer up to what the STFT and the file format round: fewer artifacts than
        # whatever a network makes of it
        print("bss cli: mixed %.2f / %.2f / %.2f  denoised %.2f / %.2f / %.2f" % tuple(rec[k][f] for k in ("mixed", "denoised")
                                                                                      for f in score.BSS_FIGURES))
        assert rec["mixed"]["sar_db"] > rec["denoised"]["sar_db"]
        assert rec["improvement"]["sir_i"] == rec["denoised"]["sir_db"] - rec["mixed"]["sir_db"]
        for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
            assert open(str(tmp_path / ("plain" + tail)), "rb").read() == open(str(tmp_path / ("scored" + tail)), "rb").read()
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "o1")] + common)
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "o2"), "--score_against", str(tgd),
                    "--score_out", str(tmp_path / "s.json"), "--bss", "--interferer", str(ifd)] + common)
        res = json.load(open(str(tmp_path / "s.json")))
        assert sorted(res["files"]) == [str(ind / "a.wav"), str(ind / "b.wav")]
        assert all(math.isfinite(f[k][fig]) for f in res["files"].values() for k in ("denoised", "mixed") for fig in ("sdr_db", "sir_db"))
        assert res["mean"]["denoised"]["sdr_db"] == pytest.approx(np.mean([f["denoised"]["sdr_db"] for f in res["files"].values()]), rel=1e-15)
        assert "sir_i" in res["mean"]["improvement"]
        _same_files(str(tmp_path / "o1"), str(tmp_path / "o2"))
        with pytest.raises(SystemExit):
            apply.main(["--input", str(ind / "a.wav"), "--output", str(tmp_path / "x.wav"), "--score_against", str(tgd / "a.wav"), "--bss"] + common)
    finally:
        apply._engines.pop("denoiser", None)
        for k in ("score_against", "score_out", "interferer"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.bss = False
        apply.FLAGS.input, apply.FLAGS.output, apply.FLAGS.neg, apply.FLAGS.pos = (apply.Flags.input, apply.Flags.output,
                                                                                    apply.Flags.neg, apply.Flags.pos)
        apply.FLAGS.weights = apply.Flags.weights
