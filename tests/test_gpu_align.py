"""Delay estimation on the device (align.hip: nhans_align, nhans_align_cut) against the float64 definition
nhans_amd.score.align_reference on identical input, within the bars of tests/align_checks.py, the delay equal on every
clip; the lag vectors bit for bit in the order the kernel states, and independent of batch, offset, run and D; the exact
clips and the tie rule; the refusals; the cut; Context.score(align=..., delays=...), Context.stoi and Context.bss_eval with
delays; the fixture of the reference's own demo pairs; the command line; the input / output contract of the calls.  Every
test prints its worst ratio to the bar (pytest -s)."""
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

import align_checks as A
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


def align_dev(eng, clips, D, pads=(0, 0)):
    """clips [(estimate, target)] aligned in one call, either buffer starting with pads[k] spare samples (of a value that
    would show in every sum) -> (records [n, 8] numpy, lag vectors [n, 2 D + 1] numpy)"""
    ten, offs = [], []
    for k in (0, 1):
        xs = [np.full(pads[k], 1e30, np.float32)] + [c[k] for c in clips]
        offs.append(np.cumsum([0] + [len(x) for x in xs]).tolist()[1:])
        ten.append(dev(np.concatenate(xs)))
    rec, corr = eng.align_device(ten[0], offs[0], ten[1], offs[1], max_lag=D, corr=True)
    return rec.cpu().numpy(), corr.cpu().numpy()


def worse(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def same_records(a, b):
    """two lists of dicts with the same keys and, figure by figure, the same bits"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y), (sorted(x), sorted(y))
        for k in x:
            assert float(x[k]).hex() == float(y[k]).hex(), (k, x[k], y[k])


@pytest.mark.parametrize("D", sorted({s[2] for s in A.SHAPES}))
def test_every_shape_within_the_bars_and_bit_equal(eng, D):
    worst = {}
    idx = [i for i, s in enumerate(A.SHAPES) if s[2] == D]
    refs = [A.shape_reference(i) for i in idx]
    clips = [(r[0], r[1]) for r in refs]
    rec, corr = align_dev(eng, clips, D, pads=(1, 3))
    assert (rec[:, 7] == 0.0).all() and not np.signbit(rec[:, 7]).any()
    D2 = min(D + 37, hip.ALIGN_MAX_LAG)
    _, wide = align_dev(eng, clips, D2, pads=(2, 1))
    for i, (e, t, ref, bars, how) in enumerate(refs):
        worse(worst, A.align_ratios(score.align_record(rec[i]), corr[i], e, t, ref, bars))
        # the order the kernel states, emulated on the host: the same bits
        assert A.same_bits(corr[i], A.device_order_corr(e, t, D)), A.SHAPES[idx[i]]
        assert int(rec[i, 6]) == eng.lib.nhans_align_common(len(e), len(t), int(rec[i, 3]))
        # alone, at aligned offsets: the same bits
        r1, c1 = align_dev(eng, [clips[i]], D)
        assert A.same_bits(r1[0], rec[i]) and A.same_bits(c1[0], corr[i]), A.SHAPES[idx[i]]
        # the shared lags of a call with a larger D
        assert A.same_bits(wide[i][D2 - D:D2 + D + 1], corr[i]), A.SHAPES[idx[i]]
    rec2, corr2 = align_dev(eng, clips, D, pads=(1, 3))
    assert A.same_bits(rec, rec2) and A.same_bits(corr, corr2)
    # another neighbourhood and another alignment: the same records
    rec3, corr3 = align_dev(eng, clips[::-1], D, pads=(2, 0))
    assert A.same_bits(rec3[::-1], rec) and A.same_bits(corr3[::-1], corr)
    print("align shapes D %d (ne, nt %s): worst ratio to the bar" % (D, ", ".join(str(A.SHAPES[i][:2]) for i in idx)), json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


def test_exact_clips_and_the_tie_rule(eng):
    clips = [A.tie_clip(k) for k in range(len(A.TIE_CLIPS))]
    D = A.TIE_CLIPS[0][3]
    got = eng.align([c[0] for c in clips], [c[1] for c in clips], max_lag=D, corr=True)
    worst = {}
    for (e, t), g, spec_ in zip(clips, got, A.TIE_CLIPS):
        ref = score.align_reference(e, t, D, corr=True)
        assert g["delay"] == spec_[4] == ref["delay"] and set(g) == set(score.ALIGN_FIELDS) | {"corr"}
        worse(worst, A.align_ratios(g, g["corr"], e, t, ref, A.corr_bars(e, t, D)))           # (exact clips: bit for bit inside)
        assert float(g["rho"]).hex() == float(ref["rho"]).hex() or (math.isnan(g["rho"]) and math.isnan(ref["rho"]))
    assert [g["delay"] for g in got] == [3, -1, 0] and math.isnan(got[2]["rho"]) and got[0]["rho"] == 1.0 / math.sqrt(2.0)
    assert not np.signbit(got[2]["corr"]).any() and (got[2]["corr"] == 0.0).all()
    assert eng.align([], []) == [] and "corr" not in eng.align(clips[0][:1], clips[0][1:], max_lag=2)[0]
    out = eng.align_device(dev(np.zeros(0, np.float32)), [0], dev(np.zeros(0, np.float32)), [0])
    assert out.shape == (0, hip.ALIGN_FIELDS)
    with pytest.raises(ValueError, match="one target per estimate"):
        eng.align([np.zeros(4, np.float32)], [])
    print("align exact clips: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) == 0.0


def test_refusals_name_the_clip_and_touch_nothing(eng):
    """Every refusal of nhans_align and nhans_align_cut with real buffers behind the pointers: afterwards no element of the
    output is written and the input holds the bits it held."""
    x = np.arange(64, dtype=np.float32)
    src = MC.Surrounded("f32", [x], [0], size=64, device=eng.device)
    before = src.host_bits().copy()
    outs = [MC.Guarded("f64", 512, which=w, device=eng.device) for w in (0, 1)]
    for g in outs:
        A.check_refusals(eng.lib, eng.handle, buf=ctypes.c_void_p(src.ptr), out=ctypes.c_void_p(g.ptr))
    torch.cuda.synchronize()
    f = MC.findings(outs, np.zeros(512, bool))
    assert not f, MC.report(f)
    assert np.array_equal(src.host_bits(), before)
    with pytest.raises(ValueError, match="not both"):
        eng.score([x], [x], align=4, delays=[0])
    with pytest.raises(ValueError, match="max_lag"):
        eng.align_device(dev(x), [0, 64], dev(x), [0, 64], max_lag=16001)


def _cut_clips():
    """pairs with delays of both signs, zero, a delay that leaves nothing, an empty clip; more than one copy tile"""
    rng = np.random.default_rng(77)
    sizes = [(5000, 4700, 211), (300, 420, -64), (9000, 9100, 0), (40, 10, 40), (0, 7, 0), (1, 1, -1), (17, 33, 5), (4097, 4096, 1)]
    return [(rng.standard_normal(ne).astype(np.float32), rng.standard_normal(nt).astype(np.float32), d) for ne, nt, d in sizes]


def test_cut_equals_the_host_slices(eng):
    clips = _cut_clips()
    es, ts, ds = [c[0] for c in clips], [c[1] for c in clips], [c[2] for c in clips]
    pad = [np.full(3, 1e30, np.float32)]
    eoff, toff = np.cumsum([3] + [len(x) for x in es]).tolist(), np.cumsum([3] + [len(x) for x in ts]).tolist()
    et, tt = dev(np.concatenate(pad + es)), dev(np.concatenate(pad + ts))
    ce, ct, off = eng.align_cut_device(et, eoff, tt, toff, ds)
    ce, ct = ce.cpu().numpy(), ct.cpu().numpy()
    for i, (e, t, d) in enumerate(clips):
        he, ht = score.align_cut(e, t, d)
        assert off[i + 1] - off[i] == len(he) == len(ht) == score.align_common(len(e), len(t), d) == eng.lib.nhans_align_common(len(e), len(t), d)
        assert MC.same_bits(ce[off[i]:off[i + 1]], he) and MC.same_bits(ct[off[i]:off[i + 1]], ht), i
    # one signal alone -- a further signal cut as the target is: the same bits, and nothing comes back for the other
    none, ct2, off2 = eng.align_cut_device(None, eoff, tt, toff, ds)
    assert none is None and off2 == off and MC.same_bits(ct2.cpu().numpy(), ct)
    ce2, none, _ = eng.align_cut_device(et, eoff, None, toff, ds)
    assert none is None and MC.same_bits(ce2.cpu().numpy(), ce)
    # the record's own delay and count drive the cut
    rec = eng.align_device(et, eoff, tt, toff, max_lag=300).cpu().numpy()
    assert all(int(r[6]) == eng.lib.nhans_align_common(len(e), len(t), int(r[3])) for r, (e, t, _) in zip(rec, clips))
    print("align cut: %d pairs, %d samples, bit-equal to the host slices: worst ratio to the bar 0" % (len(clips), off[-1]))


def test_contract_of_nhans_align_and_nhans_align_cut(eng):
    """Each call writes its documented elements and nothing beside them, and reads no sample outside the clips: three runs --
    exact sizes; guarded outputs and inputs surrounded by zeros; the other sentinel and inputs surrounded by NaN -- give
    the same bits."""
    D = 70
    pairs = [A.delayed_pair(ne, nt, d, 900 + i) for i, (ne, nt, d) in enumerate(((0, 4, 0), (1, 1, 0), (2100, 2049, 33), (300, 340, -70)))]
    pairs[1] = (np.array([0.5], np.float32), np.array([0.25], np.float32))
    sig = [[p[0] for p in pairs], [p[1] for p in pairs]]
    n, nl = len(pairs), 2 * D + 1
    p = lambda b: ctypes.c_void_p(b.ptr)
    runs, cuts = {}, {}
    for layout in ("exact", "A", "B"):
        guarded = layout != "exact"
        ins = []
        for k in (0, 1):
            off = MC.tight_offsets([len(x) for x in sig[k]])
            ins.append((MC.Surrounded("f32", sig[k], off[:-1], size=off[-1], align=(1 + k) % 4 if guarded else 0,
                                      variant="B" if layout == "B" else "A", device=eng.device), off))
        outs = [MC.Guarded("f64", size + (3 if guarded else 0), align=int(guarded), which=int(layout == "B"), device=eng.device)
                for size in (n * hip.ALIGN_FIELDS, n * nl)]
        rc = eng.lib.nhans_align(eng.handle, p(ins[0][0]), hip.i64_array(ins[0][1]), p(ins[1][0]), hip.i64_array(ins[1][1]), n, D,
                                 p(outs[0]), p(outs[1]), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        torch.cuda.synchronize()
        runs[layout] = outs
        # the cut by the delays just found, into rooms with slack between them
        rec = outs[0].region()[:n * hip.ALIGN_FIELDS].reshape(n, hip.ALIGN_FIELDS)
        delays, counts = [int(v) for v in rec[:, 3]], [int(v) for v in rec[:, 6]]
        ooff = MC.ragged_offsets(counts) if guarded else MC.tight_offsets(counts)
        co = [MC.Guarded("f32", ooff[-1], align=(2 + k) % 4 if guarded else 0, which=int(layout == "B"), device=eng.device) for k in (0, 1)]
        rc = eng.lib.nhans_align_cut(eng.handle, p(ins[0][0]), hip.i64_array(ins[0][1]), p(ins[1][0]), hip.i64_array(ins[1][1]), n,
                                     hip.i64_array(delays), p(co[0]), p(co[1]), hip.i64_array(ooff), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        torch.cuda.synchronize()
        cuts[layout] = (co, ooff, counts, delays)
    for k, size in enumerate((n * hip.ALIGN_FIELDS, n * nl)):
        mask = np.concatenate([np.ones(size, bool), np.zeros(3, bool)])
        f = MC.findings([runs["A"][k], runs["B"][k]], mask)
        assert not f, MC.report(f)
        ex, a, b = (runs[layout][k].region_bits()[:size] for layout in ("exact", "A", "B"))
        assert np.array_equal(a, ex) and np.array_equal(b, a), k
    rec = runs["exact"][0].region().reshape(n, hip.ALIGN_FIELDS)
    assert rec[:, 0].tolist() == [0, 1, 2100, 300] and rec[:, 3].tolist() == [0, 0, 33, -70] and rec[:, 6].tolist() == [0, 1, 2049, 270]
    assert cuts["A"][2:] == cuts["B"][2:] == cuts["exact"][2:]
    for k in (0, 1):
        (ga, ooff, counts, delays), gb = cuts["A"], cuts["B"][0][k]
        f = MC.findings([ga[k], gb], MC.prefix_mask(ooff, counts), ooff)
        assert not f, MC.report(f)
        for i, (e, t) in enumerate(pairs):
            want = score.align_cut(e, t, delays[i])[k]
            for g in (ga[k], gb):
                assert MC.same_bits(g.region()[ooff[i]:ooff[i] + counts[i]], want), (k, i)
        ex, xo = cuts["exact"][0][k], cuts["exact"][1]
        assert all(MC.same_bits(ex.region()[xo[i]:xo[i + 1]], score.align_cut(*pairs[i], delays[i])[k]) for i in range(n))


# ---- the surface -----------------------------------------------------------------------------------
def _shifted(e, d, rng):
    """e made d samples late (d > 0: d samples of low noise in front) or early (d < 0: its first -d samples removed)"""
    return np.concatenate([(1e-3 * rng.standard_normal(d)).astype(np.float32), e]) if d >= 0 else e[-d:]


def test_aligned_scoring_equals_scoring_the_hand_cut_pairs(eng):
    rng = np.random.default_rng(78)
    clips = [B.clip(n, 0.9, 840 + i) for i, n in enumerate((3003, 5003, 4000))]
    true = [37, -123, 0]
    es = [_shifted(c[0], d, rng) for c, d in zip(clips, true)]
    ts, ns = [c[1][0] for c in clips], [c[1][1] for c in clips]
    D = 200
    found = eng.align(es, ts, max_lag=D)
    assert [r["delay"] for r in found] == true
    cut = [score.align_cut(e, t, d) for e, t, d in zip(es, ts, true)]
    ce, ct = [c[0] for c in cut], [c[1] for c in cut]
    cn = [score.align_cut(e, x, d)[1] for e, x, d in zip(es, ns, true)]
    for kw, hand in (({}, {}), ({"stoi": True}, {"stoi": True}), ({"bss": ns}, {"bss": cn}), ({"bss": True, "stoi": True}, {"bss": True, "stoi": True})):
        want = eng.score(ce, ct, **hand)
        got = eng.score(es, ts, align=D, **kw)
        same_records(got, [dict(w, delay=d, align_rho=f["rho"]) for w, d, f in zip(want, true, found)])
        got = eng.score(es, ts, delays=true, **kw)
        same_records(got, [dict(w, delay=d) for w, d in zip(want, true)])
    # aligned, the shifted pairs score as the pairs they were made from; unaligned they do not
    plain, back = eng.score(es, ts), eng.score([c[0] for c in clips], ts)
    assert set(plain[0]) == set(score.FIELDS) | set(score.ROW_FIELDS)                      # today's keys, with neither argument
    got = eng.score(es, ts, align=D)
    assert float(got[2]["si_sdr_db"]).hex() == float(back[2]["si_sdr_db"]).hex() == float(plain[2]["si_sdr_db"]).hex()
    assert got[1]["si_sdr_db"] > plain[1]["si_sdr_db"] + 3.0 and got[0]["si_sdr_db"] > plain[0]["si_sdr_db"] + 3.0
    same_records(eng.stoi(es, ts, delays=true), [dict(w, delay=d) for w, d in zip(eng.stoi(ce, ct), true)])
    same_records(eng.bss_eval(es, ts, ns, filt_len=32, delays=true), [dict(w, delay=d) for w, d in zip(eng.bss_eval(ce, ct, cn, filt_len=32), true)])
    same_records(eng.stoi(es, ts), eng.stoi(es, ts, delays=None))
    assert eng.score([], [], align=5) == [] and eng.score([], [], delays=[]) == []
    print("align scoring: delays %s found, records bit-equal to the hand-cut pairs': worst ratio to the bar 0; SI-SDR unaligned -> aligned %s"
          % (true, ", ".join("%.2f -> %.2f" % (p["si_sdr_db"], g["si_sdr_db"]) for p, g in zip(plain, got))))


def test_fixture_of_the_reference_demo_pairs(eng):
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    D = 8000
    for ex in ("example2", "example3"):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        got = eng.align([sig["denoised"], sig["mixed"], sig["denoised"], sig["mixed"], sig["denoised"][123:], sig["mixed"][123:]],
                        [sig["target"], sig["target"], sig["target"][37:], sig["target"][37:], sig["target"], sig["target"]], max_lag=D)
        assert [r["delay"] for r in got] == [0, 0, 37, 37, -123, -123], (ex, [r["delay"] for r in got])
        n = len(sig["target"])
        assert [r["n_common"] for r in got] == [n, n, n - 37, n - 37, n - 123, n - 123]
        print("align fixture %s (D %d): delays %s, rho %s" % (ex, D, [r["delay"] for r in got], ["%.3f" % r["rho"] for r in got]))
    print("align fixture: every delay equal: worst ratio to the bar 0")


# ---- the command line ------------------------------------------------------------------------------
def test_cli_with_align_ms(eng, tmp_path, capsys):
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        clean = synth.mixture(41, 1.0)
        noise = synth.noise_context(41, 1.0)
        mixed = (clean.astype(np.int32) // 2 + noise[:len(clean)].astype(np.int32) // 4).astype(np.int16)
        wavfile.write(str(tmp_path / "in.wav"), 16000, mixed)
        wavfile.write(str(tmp_path / "neg.wav"), 16000, noise)
        wavfile.write(str(tmp_path / "tgt.wav"), 16000, (clean // 2)[37:])
        wavfile.write(str(tmp_path / "interf.wav"), 16000, (noise[:len(clean)] // 4)[37:])
        common = ["--input", str(tmp_path / "in.wav"), "--neg", str(tmp_path / "neg.wav"), "--pos", str(tmp_path / "Silent.wav"),
                  "--weights", "synthetic"]
        apply.main(common + ["--output", str(tmp_path / "plain.wav")])
        capsys.readouterr()
        apply.main(common + ["--output", str(tmp_path / "scored.wav"), "--score_against", str(tmp_path / "tgt.wav"), "--align_ms", "10",
                             "--bss", "--interferer", str(tmp_path / "interf.wav")])
        text = capsys.readouterr().out
        res = json.loads(text[text.index("{"):])
        (path, rec), = res["files"].items()
        assert rec["delay_samples"] == 37 and 0.0 < rec["align_rho"] <= 1.0
        # the figures of the hand-cut call
        den, mix = apply.wavread(str(tmp_path / "scored.wav"))[1], apply.wavread(str(tmp_path / "scored_mixed_processed.wav"))[1]
        t = apply.scaled_target(str(tmp_path / "in.wav"), str(tmp_path / "tgt.wav"))
        x = apply._reader()(str(tmp_path / "interf.wav")).astype(np.float32)
        hand = eng.score([score.align_cut(den, t, 37)[0], score.align_cut(mix, t, 37)[0]], [score.align_cut(den, t, 37)[1], score.align_cut(mix, t, 37)[1]],
                         bss=[score.align_cut(den, x, 37)[1], score.align_cut(mix, x, 37)[1]])
        for k, h in zip(("denoised", "mixed"), hand):
            assert rec[k]["delay"] == 37 and set(rec[k]) == set(h) | {"delay"}
            assert all(float(rec[k][f]).hex() == float(h[f]).hex() for f in h), k
        print("align cli: delay %d, rho %.3f, SI-SDR mixed %.2f denoised %.2f: figures bit-equal to the hand-cut call's: worst ratio to the bar 0"
              % (rec["delay_samples"], rec["align_rho"], rec["mixed"]["si_sdr_db"], rec["denoised"]["si_sdr_db"]))
        for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
            assert open(str(tmp_path / ("plain" + tail)), "rb").read() == open(str(tmp_path / ("scored" + tail)), "rb").read()
        with pytest.raises(SystemExit):
            apply.main(common + ["--output", str(tmp_path / "x.wav"), "--align_ms", "10"])
    finally:
        apply._engines.pop("denoiser", None)
        for k in ("score_against", "score_out", "interferer", "align_ms"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.bss = False
        apply.FLAGS.input, apply.FLAGS.output, apply.FLAGS.neg, apply.FLAGS.pos = (apply.Flags.input, apply.Flags.output,
                                                                                    apply.Flags.neg, apply.Flags.pos)
        apply.FLAGS.weights = apply.Flags.weights
