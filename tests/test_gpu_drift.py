"""Drift-aware alignment on the device (drift.hip: nhans_drift_track, nhans_drift_warp) against the float64 definition
(nhans_amd.score.drift_reference, drift_fit, drift_warp_reference) on identical input: the lag vectors and records bit for
bit in the order the kernel states and within the bars of tests/drift_checks.py against the exactly rounded sums; the warp
bit for bit; independent of batch, offset, order, run and radius; the input / output contract and the refusals; the
analytic clips end to end; the fallback; Context.score(align=D, drift=True); the demo pairs; the command line.  Every test
prints its worst ratio to the bar (pytest -s)."""
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

import bss_checks as BC
import drift_checks as C
import memory_checks as MC

pytestmark = pytest.mark.gpu
B, H, T = C.B, C.H, C.T


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(clips, k, pad):
    xs = [np.full(pad, 1e30, np.float32)] + [c[k] for c in clips]
    return dev(np.concatenate(xs)), np.cumsum([0] + [len(x) for x in xs]).tolist()[1:]


def track_dev(eng, clips, centres, R, pads=(0, 0)):
    """clips [(estimate, target)] tracked in one call, either buffer starting with pads[k] spare samples (of a value that
    would show in every sum) -> (records [S, 8] numpy, lag vectors [S, nl] numpy, segment offsets)"""
    (et, eoff), (tt, toff) = padded(clips, 0, pads[0]), padded(clips, 1, pads[1])
    rec, soff, corr = eng.drift_track_device(et, eoff, tt, toff, centres, radius=R, corr=True)
    return rec.cpu().numpy(), corr.cpu().numpy(), soff


def warp_dev(eng, clips, lines, pad=0):
    """clips [(estimate, target length)] warped in one call -> ([y], ranges)"""
    et, eoff = padded(clips, 0, pad)
    toff = np.cumsum([0] + [c[1] for c in clips]).tolist()
    out, off, rng = eng.drift_warp_device(et, eoff, toff, lines)
    out = out.cpu().numpy()
    return [out[off[i]:off[i + 1]] for i in range(len(clips))], rng


def worse(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def same_records(a, b):
    """two lists of dicts with the same keys and, figure by figure, the same bits"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y), (sorted(x), sorted(y))
        for k in x:
            assert float(x[k]).hex() == float(y[k]).hex() or (math.isnan(x[k]) and math.isnan(y[k])), (k, x[k], y[k])


# ---- tracking --------------------------------------------------------------------------------------
def _track_cases(R):
    """(estimate, target, centre line, what it is for): nt of no, one, one, two and three segments with ne != nt both ways;
    centres that push the lags before the estimate's first and past its last sample; a silent block; a peak at the edge."""
    cases = []
    for i, (nt, dne, d) in enumerate(((B - 1, 7, 3), (B, -5, -2), (B + H - 1, 40, 5), (B + H, -33, -4), (B + 2 * H, 19, 0))):
        e, t = C.noise_pair(nt + dne, nt, 20 + i, delay=d)
        cases.append((e, t, (float(d), 0.0), "nt %d" % nt))
    if R == 1024:
        return cases[:4] + [(cases[3][0], cases[3][1], (-float(B), 0.0), "lags before the first sample"),
                            (cases[1][0], cases[1][1], (float(B + 1500), 0.0), "lags past the last sample")]
    e, t = C.noise_pair(B + H + 60, B + H, 30, delay=9)
    cases.append((e, t, (9.0 - R, 0.0), "the peak at the upper edge of the search"))
    cases.append((e, t, (9.0 + R, 0.0), "the peak at the lower edge"))
    cases.append((e, t, (-float(B + H), 0.0), "every lag before the estimate's first sample"))
    cases.append((e, t, (-float(H), 2.0 ** -11), "half of the first block before the first sample"))
    cases.append((e, t, (float(len(e) + 5000), 0.0), "every lag past the last sample"))
    cases.append((e, t, (float(H + 70), -2.0 ** -10), "the blocks' ends past the last sample"))
    ts = np.array(C.noise_pair(B + 2 * H, B + 2 * H, 31, delay=0)[1])
    ts[H:H + B] = 0.0
    cases.append((ts + np.float32(0.01), ts, (0.0, 0.0), "a silent block between two that are not"))
    ea, ta = C.analytic_clip(B + 2 * H, 5.4, 300e-6, 30.0, 9)
    cases.append((ea, ta, (6.0, 3e-4), "an analytic clip around its own line"))
    return cases


@pytest.mark.parametrize("R", [1, 64, 1024])
def test_tracking_bit_equal_to_the_stated_order_and_within_the_bars(eng, R):
    cases = _track_cases(R)
    clips, centres = [(c[0], c[1]) for c in cases], [c[2] for c in cases]
    table = score.drift_library_table()
    rec, corr, soff = track_dev(eng, clips, centres, R, pads=(1, 3))
    assert [soff[i + 1] - soff[i] for i in range(len(cases))] == [score.drift_segments(len(c[1])) for c in cases]
    worst, flags_seen = {}, set()
    for i, (e, t, (ca, cb), what) in enumerate(cases):
        refs = C.reference_segments(e, t, ca, cb, R, table=table)
        assert len(refs) == soff[i + 1] - soff[i], what
        for j, (ref, bars, cbar) in enumerate(refs):
            got = score.drift_segment_record(rec[soff[i] + j])
            assert bars["decided"] > 1.0, (what, j, bars["decided"])
            worse(worst, C.segment_ratios(got, corr[soff[i] + j], ref, bars, cbar))
            # the order the kernel states, restated on the host: the same bits, every field and every lag
            want, c = C.device_order_segment(e, t, j, ref["z"], R, table)
            assert C.same_bits(corr[soff[i] + j], c), (what, j)
            assert C.same_bits(rec[soff[i] + j], [want[k] for k in score.DRIFT_FIELDS]), (what, j, got, want)
            assert want["k"] == ref["k"]
            flags_seen.add(got["flags"])
    assert rec[:, 7].tolist() == [z for c in cases for z in score.drift_centres(c[2][0], c[2][1], score.drift_segments(len(c[1])))]
    if R != 1024:
        assert {0, score.DRIFT_EDGE, score.DRIFT_SILENT} <= flags_seen, flags_seen
    # alone, at aligned offsets; again; in reversed order beside other neighbours at another alignment: the same bits
    for i in range(len(cases)):
        r1, c1, _ = track_dev(eng, [clips[i]], [centres[i]], R)
        assert C.same_bits(r1, rec[soff[i]:soff[i + 1]]) and C.same_bits(c1, corr[soff[i]:soff[i + 1]]), cases[i][3]
    rec2, corr2, _ = track_dev(eng, clips, centres, R, pads=(1, 3))
    assert C.same_bits(rec, rec2) and C.same_bits(corr, corr2)
    rec3, corr3, soff3 = track_dev(eng, clips[::-1], centres[::-1], R, pads=(2, 0))
    n = len(cases)
    for i in range(n):
        a, b = soff3[n - 1 - i], soff3[n - i]
        assert C.same_bits(rec3[a:b], rec[soff[i]:soff[i + 1]]) and C.same_bits(corr3[a:b], corr[soff[i]:soff[i + 1]]), cases[i][3]
    # the shared lags of a call with another radius: c[d] is a function of the pair, the segment and d alone
    R2 = R + 5 if R < 1024 else R - 7
    _, wide, _ = track_dev(eng, clips, centres, R2, pads=(0, 2))
    lo = max(R2 - R, 0)
    a, b = (wide[:, lo:lo + corr.shape[1]], corr) if R2 > R else (wide, corr[:, R - R2:R - R2 + wide.shape[1]])
    assert C.same_bits(a, b)
    print("drift tracking R %d (%d clips, %d segments): worst ratio to the bar" % (R, len(cases), soff[-1]), json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


# ---- the warp --------------------------------------------------------------------------------------
def _warp_cases():
    """(estimate, target length, (a, b)): ne of 0, 1 and 2 T, a of both signs, b of 0 and +-2^-10, an empty range, a range of one
    sample, more than one workgroup, ranges that end at the estimate's end and at the target's"""
    rng = np.random.default_rng(91)
    x = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    S = 2.0 ** -10
    return [(x(0), 10, (0.0, 0.0)), (x(1), 10, (0.0, 0.0)), (x(1), 10, (-3.0, 0.0)), (x(1), 10, (0.5, 0.0)), (x(2 * T), 50, (-10.0, 0.0)),
            (x(2 * T), 40, (3.25, S)), (x(2 * T), 40, (-3.25, -S)), (x(100), 100, (200.0, 0.0)), (x(100), 100, (-200.0, 0.0)),
            (x(5000), 5000, (-2.0, S)), (x(5000), 6000, (4.0, -S)), (x(4097), 5000, (-1.0, 1.0 / 4096)), (x(3000), 3000, (-2048.5, 2.0 ** -12)),
            (x(2000), 1200, (-23.0023, 1e-4)), (x(3100), 3000, (37.3, 50e-6)), (x(3000), 3100, (-20.75, -200e-6)), (x(1025), 1024, (0.0, 0.0)),
            (x(700), 2000, (17.0, 0.0)), (x(2000), 700, (-9.0, 0.0))]


def test_warp_bit_equal_to_the_restated_chain(eng):
    cases = _warp_cases()
    table = score.drift_library_table()
    clips, lines = [(c[0], c[1]) for c in cases], [c[2] for c in cases]
    ys, rngs = warp_dev(eng, clips, lines, pad=3)
    sizes = set()
    for (e, nt, (a, b)), y, r in zip(cases, ys, rngs):
        want, lo, hi = score.drift_warp_reference(e, nt, a, b, table=table)
        assert r == (lo, hi) == C.brute_range(len(e), nt, a, b), (len(e), nt, a, b, r)
        assert C.same_f32(y, want), (len(e), nt, a, b)
        sizes.add(hi - lo)
        if b == 0.0 and a == int(a) and hi > lo:                    # an integer line is the whole-sample cut, bit for bit
            assert (lo, hi - lo) == (max(-int(a), 0), score.align_common(len(e), nt, int(a)))
            assert C.same_f32(y, score.align_cut(e, np.zeros(nt, np.float32), int(a))[0])
    assert {0, 1} <= sizes and max(sizes) > 2 * hip.DRIFT_WARP_TILE
    # alone; again; reversed beside other neighbours at another alignment: the same bits
    for i in range(len(cases)):
        y1, r1 = warp_dev(eng, [clips[i]], [lines[i]])
        assert r1 == [rngs[i]] and C.same_f32(y1[0], ys[i])
    y2, _ = warp_dev(eng, clips, lines, pad=3)
    y3, r3 = warp_dev(eng, clips[::-1], lines[::-1], pad=2)
    assert r3[::-1] == rngs and all(C.same_f32(p, q) and C.same_f32(p, s) for p, q, s in zip(ys, y2, y3[::-1]))
    assert eng.drift_warp([], [], []) == [] and eng.drift_track([], [], []) == []
    print("drift warp: %d clips, %d samples, bit-equal to the restated chain: worst ratio to the bar 0" % (len(cases), sum(len(y) for y in ys)))


# ---- the input / output contract -----------------------------------------------------------------------
def test_refusals_name_the_clip_and_touch_nothing(eng):
    x = np.arange(64, dtype=np.float32)
    src = MC.Surrounded("f32", [x], [0], size=64, device=eng.device)
    before = src.host_bits().copy()
    outs = [MC.Guarded("f64", 512, which=w, device=eng.device) for w in (0, 1)]
    for g in outs:
        C.check_refusals(eng.lib, eng.handle, buf=ctypes.c_void_p(src.ptr), out=ctypes.c_void_p(g.ptr))
    torch.cuda.synchronize()
    f = MC.findings(outs, np.zeros(512, bool))
    assert not f, MC.report(f)
    assert np.array_equal(src.host_bits(), before)
    with pytest.raises(ValueError, match="drift=True"):
        eng.score([x], [x], drift=True)
    with pytest.raises(ValueError, match="radius"):
        eng.drift_track_device(dev(x), [0, 64], dev(x), [0, 64], [(0.0, 0.0)], radius=1025)
    with pytest.raises(hip.NhansError, match="2\\^-10"):
        eng.drift_warp([x], [64], [(0.0, 0.01)])


def test_contract_of_nhans_drift_track_and_nhans_drift_warp(eng):
    """Each call writes its documented elements and nothing beside them, and reads no sample outside the clips: three runs --
    exact sizes; guarded outputs and inputs surrounded by zeros; the other sentinel and inputs surrounded by NaN -- give
    the same bits."""
    R = 5
    pairs = [C.noise_pair(B + H + 9, B + H, 40, delay=3), C.noise_pair(B - 1, B - 1, 41, delay=0), C.noise_pair(B - 40, B, 42, delay=-2),
             C.noise_pair(600, B + 2 * H, 43, delay=1)]
    centres = [(3.0, 0.0), (0.0, 0.0), (-2.0, 2.0 ** -11), (-float(H), 0.0)]       # (clips 2 and 3: lags on either side of the estimate)
    lines = [(3.0, 1e-4), (0.5, 0.0), (-2.5, -2.0 ** -10), (700.0, 0.0)]           # (clip 3: an empty range)
    sig = [[p[0] for p in pairs], [p[1] for p in pairs]]
    n, nl = len(pairs), 2 * (R + T) + 1
    S = sum(score.drift_segments(len(p[1])) for p in pairs)
    rngs = [hip.drift_range(len(p[0]), len(p[1]), *l) for p, l in zip(pairs, lines)]
    counts = [hi - lo for lo, hi in rngs]
    assert S == 2 + 0 + 1 + 3 and counts[3] == 0 and min(counts[:3]) > 0
    p = lambda b: ctypes.c_void_p(b.ptr)
    dbl = hip.dbl_array
    runs, warps = {}, {}
    for layout in ("exact", "A", "B"):
        guarded = layout != "exact"
        ins = []
        for k in (0, 1):
            off = MC.tight_offsets([len(x) for x in sig[k]])
            ins.append((MC.Surrounded("f32", sig[k], off[:-1], size=off[-1], align=(1 + k) % 4 if guarded else 0,
                                      variant="B" if layout == "B" else "A", device=eng.device), off))
        outs = [MC.Guarded("f64", size + (3 if guarded else 0), align=int(guarded), which=int(layout == "B"), device=eng.device)
                for size in (S * hip.DRIFT_FIELDS, S * nl)]
        rc = eng.lib.nhans_drift_track(eng.handle, p(ins[0][0]), hip.i64_array(ins[0][1]), p(ins[1][0]), hip.i64_array(ins[1][1]), n,
                                       dbl(c[0] for c in centres), dbl(c[1] for c in centres), R, p(outs[0]), p(outs[1]), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        torch.cuda.synchronize()
        runs[layout] = outs
        ooff = MC.ragged_offsets(counts) if guarded else MC.tight_offsets(counts)
        wo = MC.Guarded("f32", ooff[-1], align=2 if guarded else 0, which=int(layout == "B"), device=eng.device)
        rc = eng.lib.nhans_drift_warp(eng.handle, p(ins[0][0]), hip.i64_array(ins[0][1]), hip.i64_array(ins[1][1]), n,
                                      dbl(l[0] for l in lines), dbl(l[1] for l in lines), p(wo), hip.i64_array(ooff), eng._stream())
        assert rc == 0, eng.lib.nhans_last_error()
        torch.cuda.synchronize()
        warps[layout] = (wo, ooff)
    for k, size in enumerate((S * hip.DRIFT_FIELDS, S * nl)):
        mask = np.concatenate([np.ones(size, bool), np.zeros(3, bool)])
        f = MC.findings([runs["A"][k], runs["B"][k]], mask)
        assert not f, MC.report(f)
        ex, a, b = (runs[layout][k].region_bits()[:size] for layout in ("exact", "A", "B"))
        assert np.array_equal(a, ex) and np.array_equal(b, a), k
    (ga, ooff), gb = warps["A"], warps["B"][0]
    f = MC.findings([ga, gb], MC.prefix_mask(ooff, counts), ooff)
    assert not f, MC.report(f)
    table = score.drift_library_table()
    ex, xo = warps["exact"]
    for i, ((e, t), l) in enumerate(zip(pairs, lines)):
        want = score.drift_warp_reference(e, len(t), l[0], l[1], table=table)[0]
        for g, o in ((ga, ooff), (gb, ooff), (ex, xo)):
            assert MC.same_bits(g.region()[o[i]:o[i] + counts[i]], want), i
    print("drift contract: %d segments, %d warped samples: no guard word, no slack element written, no hole; the same bits in "
          "three layouts: worst ratio to the bar 0" % (S, sum(counts)))


# ---- end to end ------------------------------------------------------------------------------------
def _truth_bars():
    """twice the worst error of the REFERENCE against the true lines over the clip list (tests/test_drift_host.py prints
    each): what the algorithm itself leaves, with a margin for the spread across noise seeds"""
    ea = max(abs(C.reference_line(i)[0]["a"] - C.E2E_CLIPS[i][1]) for i in range(len(C.E2E_CLIPS)))
    eb = max(abs(C.reference_line(i)[0]["b"] - C.E2E_CLIPS[i][2]) for i in range(len(C.E2E_CLIPS)))
    return 2.0 * ea, 2.0 * eb


def test_analytic_clips_end_to_end(eng):
    table = score.drift_library_table()
    bar_ta, bar_tb = _truth_bars()
    worst = {}
    for i, (n, a, b, snr, seed, max_lag, track_lag) in enumerate(C.E2E_CLIPS):
        e, t = C.e2e_clip(i)
        fit, refs, R, centre = C.reference_line(i)
        got = eng.align_drift([e], [t], max_lag=max_lag, track_lag=track_lag)[0]
        assert got["fit_ok"] == 1 == fit["fit_ok"] and got["delay_int"] == fit["d0"] and got["segments"] == len(refs) == score.drift_segments(n)
        assert got["segments_used"] == fit["n_used"] >= 0.8 * len(refs)
        assert set(got) == {"delay", "drift", "drift_ppm", "fit_ok", "segments", "segments_used", "rms_residual", "rho", "delay_int"}
        bar_a, bar_b = C.fit_bar(refs)
        r = {"a": C.ratio(got["delay"], fit["a"], bar_a), "b": C.ratio(got["drift"], fit["b"], bar_b),
             "a_truth": abs(got["delay"] - a) / bar_ta, "b_truth": abs(got["drift"] - b) / bar_tb}
        worse(worst, r)
        # the warped pair: the device's warp is the restated chain, and scoring it is scoring the hand-warped pair
        (y, lo, hi), = eng.drift_warp([e], [n], [(got["delay"], got["drift"])])
        want, wlo, whi = score.drift_warp_reference(e, n, got["delay"], got["drift"], table=table)
        assert (lo, hi) == (wlo, whi) and C.same_f32(y, want), i
        hand = eng.score([want], [t[wlo:whi]])[0]                   # (the pair warped on the host)
        whole = eng.score([e], [t], align=max_lag)[0]
        if track_lag == 64:
            rec = eng.score([e], [t], align=max_lag, drift=True)[0]
            same_records([rec], [dict(hand, delay=got["delay"], drift_ppm=got["drift_ppm"], drift_ok=1, align_rho=got["rho"])])
        assert hand["si_sdr_db"] > whole["si_sdr_db"] + 3.0, (i, hand["si_sdr_db"], whole["si_sdr_db"])
        print("drift clip %d (%.1f s, %.1f ppm, %g dB): line (%.4f, %.3f ppm) against the reference's (%.4f, %.3f ppm) and the true "
              "(%.4f, %.1f ppm); used %d / %d; SI-SDR whole-sample %.2f dB, warped %.2f dB; ratios %s"
              % (i, n / 16000.0, 1e6 * b, snr, got["delay"], got["drift_ppm"], fit["a"], 1e6 * fit["b"], a, 1e6 * b, got["segments_used"],
                 got["segments"], whole["si_sdr_db"], hand["si_sdr_db"], json.dumps(r)))
    # the narrow first pass alone reaches only the middle of the long clip: the second pass is what recovers its ends
    e, t = C.e2e_clip(4)
    first = eng.drift_fit(eng.drift_track([e], [t], [(float(C.reference_line(4)[0]["d0"]), 0.0)], radius=8)[0])
    assert first["fit_ok"] == 1 and first["n_valid"] < 0.8 * score.drift_segments(len(t)), first
    print("drift end to end (truth bars: %.4f sample, %.3f ppm): worst ratio to the bar" % (bar_ta, 1e6 * bar_tb), json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


def test_fallback_is_the_whole_sample_cut(eng):
    """A clip of fewer than three blocks and a clip of independent noise: no fit, and the records are those of align=D bit for
    bit, plus the new keys."""
    short = C.analytic_clip(B + 2 * H - 1, 4.3, 100e-6, 30.0, 12)
    noise = C.noise_pair(20000, 20000, 50)
    es, ts = [short[0], noise[0]], [short[1], noise[1]]
    lines = eng.align_drift(es, ts, max_lag=100)
    assert [l["fit_ok"] for l in lines] == [0, 0] and [l["segments"] for l in lines] == [2, 8]
    assert all(l["delay"] == float(l["delay_int"]) and l["drift"] == 0.0 and l["drift_ppm"] == 0.0 for l in lines)
    assert lines[0]["segments_used"] == 2 and lines[1]["segments_used"] == 0
    for kw in ({}, {"stoi": True, "quality": True}):
        whole = eng.score(es, ts, align=100, **kw)
        got = eng.score(es, ts, align=100, drift=True, **kw)
        same_records(got, [dict(w, drift_ppm=0.0, drift_ok=0) for w in whole])
        assert all(isinstance(g["delay"], int) for g in got)
    print("drift fallback: two clips without a fit, records bit-equal to align=D: worst ratio to the bar 0")


def test_drift_scoring_equals_scoring_the_hand_warped_pairs(eng):
    clips = [BC.clip(n, 0.9, 860 + i) for i, n in enumerate((12003, 14003))]
    ts, ns = [c[1][0] for c in clips], [c[1][1] for c in clips]
    true = [(5.5, 200e-6), (-7.25, -120e-6)]
    # the estimates on another clock: each resampled by the reference at the inverse line (a clip of speech-like noise has
    # content up to 8 kHz, so this is a test of the plumbing, not of the figures)
    es = []
    for c, (a, b) in zip(clips, true):
        inv = score.drift_warp_reference(np.concatenate([np.zeros(40, np.float32), c[0], np.zeros(40, np.float32)]), len(c[0]) + 20,
                                         40.0 - a / (1.0 + b), 1.0 / (1.0 + b) - 1.0)
        es.append(inv[0])
    lines = eng.align_drift(es, ts, max_lag=200)
    assert [l["fit_ok"] for l in lines] == [1, 1], lines
    assert all(abs(l["delay"] - a) < 0.1 and abs(l["drift"] - b) < 20e-6 for l, (a, b) in zip(lines, true)), lines
    warped = eng.drift_warp(es, [len(t) for t in ts], [(l["delay"], l["drift"]) for l in lines])
    ye, yt = [w[0] for w in warped], [t[w[1]:w[2]] for t, w in zip(ts, warped)]
    yn = [x[w[1]:w[2]] for x, w in zip(ns, warped)]
    tags = [dict(delay=l["delay"], drift_ppm=l["drift_ppm"], drift_ok=1, align_rho=l["rho"]) for l in lines]
    for kw, hand in (({}, {}), ({"stoi": True}, {"stoi": True}), ({"bss": ns}, {"bss": yn}), ({"quality": True}, {"quality": True}),
                     ({"bss": True, "stoi": True, "quality": True}, {"bss": True, "stoi": True, "quality": True})):
        want = eng.score(ye, yt, **hand)
        got = eng.score(es, ts, align=200, drift=True, **kw)
        same_records(got, [dict(w, **tag) for w, tag in zip(want, tags)])
    # the further signal cut by nhans_align_cut as the header says: no estimate, lengths u_hi - u_lo, delay -u_lo
    xt, xoff = padded([(x,) for x in ns], 0, 0)
    fake = np.cumsum([0] + [w[2] - w[1] for w in warped]).tolist()
    _, cut, off = eng.align_cut_device(None, fake, xt, xoff, [-w[1] for w in warped])
    cut = cut.cpu().numpy()
    assert all(C.same_f32(cut[off[i]:off[i + 1]], yn[i]) for i in range(len(ns)))
    plain = eng.score(es, ts)
    assert set(plain[0]) == set(score.FIELDS) | set(score.ROW_FIELDS)                      # today's keys, without the arguments
    assert set(eng.score(es, ts, align=200)[0]) == set(plain[0]) | {"delay", "align_rho"}
    assert eng.score([], [], align=5, drift=True) == []
    print("drift scoring: lines %s, records bit-equal to the hand-warped pairs': worst ratio to the bar 0"
          % [(round(l["delay"], 3), round(l["drift_ppm"], 1)) for l in lines])


def test_both_engines_give_the_same_bits(eng, weights_denoiser):
    """Context.align_drift, drift_warp and score(drift=True) over torch memory (engine.Engine) and over the HIP runtime's
    (lite.LiteEngine): the same library, the same bits."""
    from nhans_amd import lite
    e, t = C.analytic_clip(B + 4 * H, 5.4, 300e-6, 30.0, 9)
    le = lite.LiteEngine("denoiser", weights_denoiser)
    try:
        a, b = eng.align_drift([e], [t], max_lag=100), le.align_drift([e], [t], max_lag=100)
        assert a[0]["fit_ok"] == 1 and a[0]["segments"] == a[0]["segments_used"] == 5
        same_records(a, b)
        line = [(a[0]["delay"], a[0]["drift"])]
        (y1, lo1, hi1), = eng.drift_warp([e], [len(t)], line)
        (y2, lo2, hi2), = le.drift_warp([e], [len(t)], line)
        assert (lo1, hi1) == (lo2, hi2) and C.same_f32(y1, y2)
        same_records(eng.score([e], [t], align=100, drift=True), le.score([e], [t], align=100, drift=True))
        assert le.drift_warp([], [], []) == [] and le.drift_track([], [], []) == []
    finally:
        le.close()
    print("drift, both engines: line (%.4f, %.3f ppm), records and warped samples bit-equal: worst ratio to the bar 0"
          % (a[0]["delay"], a[0]["drift_ppm"]))


def _reference_align_drift(e, t, max_lag, track_lag=64):
    d0 = C.coarse_delay(e, t, max_lag)
    refs = C.reference_segments(e, t, float(d0), 0.0, track_lag)
    fit = score.drift_fit([r[0] for r in refs])
    if fit["fit_ok"]:
        refs = C.reference_segments(e, t, fit["a"], fit["b"], 8)
        fit = score.drift_fit([r[0] for r in refs])
    return fit, refs


def test_fixture_of_the_reference_demo_pairs(eng):
    """The demo pairs have one clock: the denoised and mixed signals against the target give a line near (0, 0), and the target
    with 37 samples removed one near (37, 0) -- `near` being the reference's own value on the CPU plus the fit's bar."""
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    worst = {}
    for ex in ("example2", "example3"):
        sig = {k: g["%s_%s" % (ex, k)] for k in ("mixed", "denoised", "target")}
        es, ts = [sig["denoised"], sig["mixed"], sig["denoised"]], [sig["target"], sig["target"], sig["target"][37:]]
        got = eng.align_drift(es, ts, max_lag=400)
        for e, t, l, d in zip(es, ts, got, (0, 0, 37)):
            fit, refs = _reference_align_drift(e, t, 400)
            assert l["fit_ok"] == fit["fit_ok"] == 1 and l["delay_int"] == d, (ex, l, fit)
            bar_a, bar_b = C.fit_bar(refs)
            worse(worst, {"a": C.ratio(l["delay"], fit["a"], bar_a), "b": C.ratio(l["drift"], fit["b"], bar_b)})
            assert abs(l["delay"] - d) <= abs(fit["a"] - d) + bar_a and abs(l["drift"]) <= abs(fit["b"]) + bar_b
            assert abs(fit["a"] - d) < 0.5 and abs(fit["b"]) < 30e-6, (ex, fit)          # (the reference itself: near indeed)
            print("drift fixture %s: line (%.4f, %.3f ppm), the reference's (%.4f, %.3f ppm), used %d / %d"
                  % (ex, l["delay"], l["drift_ppm"], fit["a"], 1e6 * fit["b"], l["segments_used"], l["segments"]))
    print("drift fixture: worst ratio to the bar", json.dumps(worst))
    assert max(worst.values()) <= 1.0, worst


# ---- the command line ------------------------------------------------------------------------------
def test_cli_with_align_drift(eng, tmp_path, capsys):
    from scipy.io import wavfile
    before = eng.precision
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    try:
        clean = synth.mixture(41, 2.0)
        noise = synth.noise_context(41, 2.0)
        mixed = (clean.astype(np.int32) // 2 + noise[:len(clean)].astype(np.int32) // 4).astype(np.int16)
        # the target and the interferer on another clock: target[u] = clean at 37.5 + u + 250 ppm u, so the files written are
        # 37.5 samples late against it and run 250 ppm fast
        a, b = 37.5, 250e-6
        other = lambda x: np.round(score.drift_warp_reference(x.astype(np.float32), len(x), a, b)[0]).astype(np.int16)
        wavfile.write(str(tmp_path / "in.wav"), 16000, mixed)
        wavfile.write(str(tmp_path / "neg.wav"), 16000, noise)
        wavfile.write(str(tmp_path / "tgt.wav"), 16000, other(clean // 2))
        wavfile.write(str(tmp_path / "interf.wav"), 16000, other(noise[:len(clean)] // 4))
        common = ["--input", str(tmp_path / "in.wav"), "--neg", str(tmp_path / "neg.wav"), "--pos", str(tmp_path / "Silent.wav"),
                  "--weights", "synthetic"]
        apply.main(common + ["--output", str(tmp_path / "plain.wav")])
        capsys.readouterr()
        apply.main(common + ["--output", str(tmp_path / "scored.wav"), "--score_against", str(tmp_path / "tgt.wav"), "--align_ms", "10",
                             "--align_drift", "--bss", "--interferer", str(tmp_path / "interf.wav")])
        text = capsys.readouterr().out
        res = json.loads(text[text.index("{"):])
        (path, rec), = res["files"].items()
        # the figures of the hand call
        den, mix = apply.wavread(str(tmp_path / "scored.wav"))[1], apply.wavread(str(tmp_path / "scored_mixed_processed.wav"))[1]
        t = apply.scaled_target(str(tmp_path / "in.wav"), str(tmp_path / "tgt.wav"))
        x = apply._reader()(str(tmp_path / "interf.wav")).astype(np.float32)
        line = eng.align_drift([den], [t], max_lag=160)[0]
        assert line["fit_ok"] == 1 and rec["drift_ok"] == 1
        assert float(rec["delay_samples"]).hex() == float(line["delay"]).hex() and float(rec["drift_ppm"]).hex() == float(line["drift_ppm"]).hex()
        assert float(rec["align_rho"]).hex() == float(line["rho"]).hex()
        w = eng.drift_warp([den, mix], [len(t), len(t)], [(line["delay"], line["drift"])] * 2)
        hand = eng.score([w[0][0], w[1][0]], [t[w[0][1]:w[0][2]], t[w[1][1]:w[1][2]]], bss=[x[w[0][1]:w[0][2]], x[w[1][1]:w[1][2]]])
        for k, h in zip(("denoised", "mixed"), hand):
            assert set(rec[k]) == set(h)
            assert all(float(rec[k][f]).hex() == float(h[f]).hex() for f in h), k
        print("drift cli: line (%.4f, %.3f ppm) for a target made with (%.1f, %.1f ppm), rho %.3f, SI-SDR mixed %.2f denoised %.2f: figures "
              "bit-equal to the hand call's: worst ratio to the bar 0" % (rec["delay_samples"], rec["drift_ppm"], a, 1e6 * b, rec["align_rho"],
                                                                          rec["mixed"]["si_sdr_db"], rec["denoised"]["si_sdr_db"]))
        assert abs(rec["delay_samples"] - a) < 0.5 and abs(rec["drift_ppm"] - 1e6 * b) < 30.0
        for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
            assert open(str(tmp_path / ("plain" + tail)), "rb").read() == open(str(tmp_path / ("scored" + tail)), "rb").read()
        with pytest.raises(SystemExit):
            apply.main(common + ["--output", str(tmp_path / "x.wav"), "--score_against", str(tmp_path / "tgt.wav"), "--align_drift"])
    finally:
        apply._engines.pop("denoiser", None)
        for k in ("score_against", "score_out", "interferer", "align_ms"):
            setattr(apply.FLAGS, k, None)
        apply.FLAGS.bss = False
        apply.FLAGS.align_drift = False
        eng.set_precision(before)
        apply.FLAGS.input, apply.FLAGS.output, apply.FLAGS.neg, apply.FLAGS.pos = (apply.Flags.input, apply.Flags.output,
                                                                                    apply.Flags.neg, apply.Flags.pos)
        apply.FLAGS.weights = apply.Flags.weights
