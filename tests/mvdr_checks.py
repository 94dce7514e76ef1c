"""Shared pieces of the MVDR tests (tests/test_gpu_mvdr.py on the device, tests/test_mvdr_host.py for the CPU half): the
simulated array scenes built from tests/golden/score_demo_pairs.npz, the float64 definition (nhans_amd.mvdr) with the
faults planted in copies of it, and the bars of the teacher-forced stage checks.

Scenes (simulated, free field).  A point target and a point interferer reach a line of C microphones with a delay per
microphone: the target image is the fixture's target delayed 0.37 c samples at microphone c, the interferer is mixed -
a target (a the least-squares factor) delayed -1.21 c samples, both by a 33-tap Kaiser (beta 8.6) windowed sinc; white
sensor noise of standard deviation 1e-3 is added.  The reference is channel 0, where both delays are 0.  The trained
mask is min(1, |STFT(denoised)| / |STFT(mixed)|) of the fixture's own signals, the oracle mask the ratio mask of the two
images at channel 0.  All transforms are the library's pair (nhans_amd.phase.analyse / synthesise).  Scores are SI-SDR
against the target's image at channel 0 over the INTERIOR of the clip, the first and last EDGE = 400 samples left out:
the synthesis window keeps the edges bounded, but the first and last 240 samples lie under fewer than three frames and
are not reconstructed, which costs every estimate that went through the transform pair and none that did not.

Bars.  Every stage is teacher-forced: the reference takes the device's own output of the stage before, so a bar holds
the roundings of one stage only.  u = 2^-53.
  spectra      tests/stft_checks.py's frame bar on the complex values: K ratio max_k|X| + A, ratio that of the float32 CPU
               restatement (torch rfft) against float64.
  covariances  entry (i, j): p = x_i conj(x_j) has one rounding per part (products of float32 are exact in double), the
               fma chain one rounding of the partial sum per frame -- at most (T + 1) u S per part on the device, S = sum_t
               m |x_i| |x_j|; 1 - m is exact or one rounding more; numpy's own sum as much again; the modulus of two parts
               sqrt 2: 4 (T + 4) u S, plus the smallest double for an S of zero.
  weights      the teacher is the definition in extended precision (np.clongdouble) on the device's covariances.  A
               Cholesky solve is backward stable: (A + dA) g = b with ||dA|| <= C gamma_{3C+1} ||A|| (Higham, Accuracy and
               Stability, thm 10.4), complex arithmetic costing a factor below 4 (lemma 3.5), the loading and the trace
               (C + 2) u more: eps = 4 C (3 C + 2) u cond_2(Phi_n') bounds ||dg|| / ||g|| to first order.  Then
               ||dw|| <= (eps ||g_ref|| + ||w|| (eps sum_j ||g_j|| + C u sum_j |g_jj|)) / tau + u ||w||.  Where eps >= 1/4 the
               pivots' signs are rounding themselves -- the definition in float64 could not say either whether the bin
               falls back -- and the bin is left out of the comparison of w and of the fallback flags (counted and printed).
  filter       y against the double sum of the device's X and w: half an ulp of float32 in each part, 2^-24 |y|, plus the
               four fma per channel in double, 8 C u sum_c |w_c| |x_c|, plus the smallest float32 sub-normal.
  rows         lm against ln max(|y|, 1e-5) of the device's own y: squares, sum and root 2.5 ulp of |y|, the hardware log2
               1 ulp and the product by ln 2 half an ulp of lm: 2^-22 (1 + |lm|).  ph against atan2 of the device's y: the
               fit's 1.7e-7 rad and the roundings of its evaluation, 4e-7, wrapped; not where both parts are below the
               smallest normal float32 (the header: such a bin has the phase of an axis).
"""
import os

import numpy as np
import torch

import nhans_amd  # noqa: F401
from nhans_amd import mvdr, phase

import stft_checks as S

WIN, HOP, BINS = mvdr.WIN, mvdr.HOP, mvdr.BINS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EDGE = 400
U = 2.0 ** -53
TARGET_DELAY, INTERFERER_DELAY, SENSOR_NOISE = 0.37, -1.21, 1e-3
TAPS, BETA = 33, 8.6
SCENES = ("example2", "example3")
MARGIN_DB = 3.0                             # the condition: see test_mvdr_host.py
# exp of a log-gain on the device (nhans_istft's): the hardware exp2 1 ulp, the correction factor and the product half an
# ulp each -- 2 ulp of float32
EXP_REL = 2.0 ** -22
COUNTS = (1, 2, 3, 63, 64, 65, 138)         # frames: the edges of a 64-way split of the frames, and the fixture's clip


# ---- scenes ------------------------------------------------------------------------------------------------------
def frac_delay(x, d):
    """x delayed by d samples (any real d, |d| < 12) with a 33-tap Kaiser windowed sinc; same length, float64."""
    n = np.arange(TAPS) - TAPS // 2
    h = np.sinc(n - d) * np.kaiser(TAPS, BETA)
    return np.convolve(np.asarray(x, dtype=np.float64), h)[TAPS // 2:TAPS // 2 + len(x)]


_fixture = {}


def fixture():
    if not _fixture:
        _fixture.update(np.load(os.path.join(GOLDEN, "score_demo_pairs.npz")))
    return _fixture


def array_scene(target, interferer, C, seed):
    """-> dict: x float32 [n, C], target_image and interferer_image float64 [n] (channel 0)."""
    rng = np.random.default_rng(seed)
    s = np.stack([frac_delay(target, TARGET_DELAY * c) for c in range(C)], axis=1)
    v = np.stack([frac_delay(interferer, INTERFERER_DELAY * c) for c in range(C)], axis=1)
    x = s + v + SENSOR_NOISE * rng.standard_normal(s.shape)
    return {"x": x.astype(np.float32), "target_image": s[:, 0], "interferer_image": v[:, 0], "C": C}


def scene(name, C):
    """The scene of a fixture triple with C microphones, and its two masks [T, 201] float32."""
    g = fixture()
    tgt, mix, den = (g["%s_%s" % (name, k)].astype(np.float64) for k in ("target", "mixed", "denoised"))
    a = float(mix @ tgt) / float(tgt @ tgt)
    sc = array_scene(tgt, mix - a * tgt, C, 9000 + C)
    num, dn = np.abs(phase.analyse(den)), np.abs(phase.analyse(mix))
    sc["trained_mask"] = np.minimum(1.0, np.divide(num, dn, out=np.ones_like(num), where=dn > 0)).astype(np.float32)
    sc["oracle_mask"] = ratio_mask(sc["target_image"], sc["interferer_image"])
    sc["name"] = name
    return sc


def two_speaker_scene(C):
    """The two fixture targets against each other at 0 dB."""
    g = fixture()
    a, b = g["example2_target"].astype(np.float64), g["example3_target"].astype(np.float64)
    n = min(len(a), len(b))
    n = WIN + HOP * ((n - WIN) // HOP)
    a, b = a[:n], b[:n]
    b = b * np.sqrt((a @ a) / (b @ b))
    sc = array_scene(a, b, C, 9100 + C)
    sc["oracle_mask"] = ratio_mask(sc["target_image"], sc["interferer_image"])
    sc["poor_mask"] = (0.25 + 0.5 * sc["oracle_mask"]).astype(np.float32)
    sc["name"] = "two speakers"
    return sc


def ratio_mask(s, v):
    ms, mv = np.abs(phase.analyse(s)), np.abs(phase.analyse(v))
    return np.divide(ms, ms + mv, out=np.ones_like(ms), where=ms + mv > 0).astype(np.float32)


def interior(x):
    return np.asarray(x)[EDGE:len(x) - EDGE]


def si_sdr(est, tgt):
    """SI-SDR in dB over the interior of the common prefix."""
    n = min(len(est), len(tgt))
    return phase.si_sdr(interior(est[:n]), interior(tgt[:n]))


def masked_reference_channel(x, mask, ref=0):
    """The mask alone on the reference channel -> waveform (float64)."""
    return phase.synthesise(mvdr.mask_values(mask) * phase.analyse(np.asarray(x, dtype=np.float64)[:, ref]))


def scene_scores(sc, mask, reference=mvdr.reference, ref=0, loading=mvdr.LOADING):
    """The float64 figures of one scene and mask: SI-SDR of channel `ref`, the channel mean, the mask alone on channel `ref`
    and the MVDR output, and the bins that fell back."""
    x = sc["x"].astype(np.float64)
    r = reference(sc["x"], mask, ref=ref, loading=loading)
    t = sc["target_image"]
    return {"ref": si_sdr(x[:, ref], t), "mean": si_sdr(x.mean(axis=1), t), "mask": si_sdr(masked_reference_channel(x, mask, ref), t),
            "mvdr": si_sdr(phase.synthesise(r["y"]), t), "fallback_bins": int(r["record"]["fallback_bins"])}


# ---- planted faults: copies of the definition, each wrong in one place ---------------------------------------------
def reference_transposed(x, mask, ref=0, loading=mvdr.LOADING):
    """w^T x in place of w^H x."""
    r = mvdr.reference(x, mask, ref=ref, loading=loading)
    r["y"] = mvdr.apply(r["X"], np.conj(r["w"]))
    return r


def reference_masks_swapped(x, mask, ref=0, loading=mvdr.LOADING):
    """Phi_s and Phi_n trade places."""
    X = mvdr.spectra(x)
    ps, pn = mvdr.covariances(X, mvdr.mask_values(mask))
    w, fb = mvdr.weights(pn, ps, ref, loading)
    return {"X": X, "w": w, "y": mvdr.apply(X, w), "fallback": fb, "record": {"fallback_bins": float(fb.sum())}}


# ---- small cases for the stage checks -------------------------------------------------------------------------------
def random_clip(T, C, seed, tail=0):
    """A clip of T frames (and `tail` < 160 untrimmed samples): a common source with per-channel gains and delays plus
    noise of its own, so that the covariances have structure; float32 [n, C]."""
    rng = np.random.default_rng(seed)
    n = WIN + HOP * (T - 1) + tail
    src, jam = rng.standard_normal(n + 8), rng.standard_normal(n + 8)
    x = np.stack([(1.0 + 0.1 * c) * src[c % 4:c % 4 + n] + 0.7 * jam[(3 * c) % 5:(3 * c) % 5 + n] + 0.05 * rng.standard_normal(n)
                  for c in range(C)], axis=1)
    return (0.1 * x).astype(np.float32)


def random_mask(T, seed, loggain=False):
    rng = np.random.default_rng(seed)
    m = rng.uniform(-0.2, 1.2, (T, BINS))           # both clamps are reached
    if loggain:
        m = np.log(np.maximum(rng.uniform(-0.2, 1.5, (T, BINS)), 1e-3))      # some gains above 0
    return m.astype(np.float32)


# ---- the bars ------------------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def cpu32_spectrum(wav):
    """torch.fft.rfft of the float32 windowed frames: complex64 [T, 201]."""
    return torch.fft.rfft(S._frames32(wav), n=WIN, dim=1).numpy()


_ratios = {}


def spectrum_ratio(key, wavs):
    """The restatement's largest max_k|X32 - X64| / max_k|X64| over the frames of `wavs` (tests/stft_checks.py's ratio)."""
    if key not in _ratios:
        r = 0.0
        for w in wavs:
            X = phase.analyse(w)
            err, mx = np.abs(cpu32_spectrum(w) - X).max(axis=1), np.abs(X).max(axis=1)
            ok = mx >= S.TINY
            if ok.any():
                r = max(r, float((np.maximum(err[ok] - S.A, 0.0) / mx[ok]).max()))
        _ratios[key] = r
    return _ratios[key]


def check_spectra(label, X_dev, x, ratio):
    """X_dev complex64 [C, T, 201] of the clip x [n, C] -> Verdict(ok, message, rel: the largest err / bar)."""
    worst, msg = 0.0, ""
    if not S.K * ratio < S.CAP_ANALYSIS:
        return Verdict(ok=False, message="%s: the bar %g x %.3e is not below the cap" % (label, S.K, ratio), rel=np.inf)
    for c in range(x.shape[1]):
        X = phase.analyse(x[:, c])
        d = np.abs(X_dev[c].astype(np.complex128) - X)
        d[~np.isfinite(d)] = np.inf
        mx = np.abs(X).max(axis=1)
        bar = np.where(mx >= S.TINY, S.K * ratio * mx, 0.0) + S.A
        rel = d.max(axis=1) / bar
        if len(rel) and rel.max() > worst:
            worst = float(rel.max())
            f = int(rel.argmax())
            msg = "%s: channel %d frame %d bin %d: |X - X64| = %.3e for the bar %.3e" % (label, c, f, int(d[f].argmax()), d[f].max(), bar[f])
    return Verdict(ok=worst <= 1.0, message=msg, rel=worst)


def check_covariances(label, ps_dev, pn_dev, X_dev, m, mask_rel=0.0):
    """The device's Phi_s, Phi_n [201, C, C] against the definition on the device's own X [C, T, 201] and m [T, 201].  mask_rel:
    how far the device's own m may be from the definition's, relative to m (EXP_REL for log-gain rows): it moves an entry of
    Phi_s by that share of S, and one of Phi_n by that share of sum_t m |x_i| |x_j| as well (d(1 - m) = -dm)."""
    Xd = X_dev.astype(np.complex128)
    T = Xd.shape[1]
    ps, pn = mvdr.covariances(Xd, m)
    a = np.abs(Xd)                                                  # [C, T, K]
    worst, msg = 0.0, ""
    for name, got, want, wt in (("Phi_s", ps_dev, ps, m), ("Phi_n", pn_dev, pn, 1.0 - m)):
        Sij = np.einsum("tk,itk,jtk->kij", wt, a, a)
        bar = 4.0 * (T + 4) * U * Sij + mask_rel * np.einsum("tk,itk,jtk->kij", m, a, a) + np.finfo(np.float64).tiny
        d = np.abs(got - want)
        d[~np.isfinite(d)] = np.inf
        rel = d / bar
        if rel.max() > worst:
            worst = float(rel.max())
            k, i, j = np.unravel_index(int(rel.argmax()), rel.shape)
            msg = "%s: %s bin %d entry (%d, %d): off by %.3e for the bar %.3e" % (label, name, k, i, j, d[k, i, j], bar[k, i, j])
        herm = np.abs(got - np.conj(got.transpose(0, 2, 1))).max()
        if herm != 0.0 or np.abs(np.diagonal(got, axis1=1, axis2=2).imag).max() != 0.0:
            return Verdict(ok=False, message="%s: %s is not exactly Hermitian with a real diagonal" % (label, name), rel=np.inf)
    return Verdict(ok=worst <= 1.0, message=msg, rel=worst)


def check_weights(label, w_dev, ps_dev, pn_dev, ref, loading):
    """The device's w [201, C] against the extended-precision teacher on the device's own covariances.  Verdict: ok, message,
    rel (largest err / bar over the judged bins), fallback (the teacher's flags), judged (bool [201])."""
    C = w_dev.shape[1]
    w_t, fb_t = mvdr.weights(ps_dev, pn_dev, ref, loading, dtype=np.clongdouble)
    w_t = w_t.astype(np.complex128)
    tr = np.einsum("kii->k", pn_dev).real
    A = pn_dev + (loading * tr / C)[:, None, None] * np.eye(C)[None]
    finite = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(ps_dev).all(axis=(1, 2))
    cond = np.full(BINS, np.inf)
    G = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for k in np.flatnonzero(finite & (tr != 0)):
            sv = np.linalg.svd(A[k], compute_uv=False)
            if sv[-1] > 0:
                cond[k] = sv[0] / sv[-1]
                if cond[k] * U < 0.25:
                    G[k] = np.linalg.solve(A[k], ps_dev[k])
    eps = 4.0 * C * (3 * C + 2) * U * cond
    sure = (tr == 0) & finite                        # tr = 0 is exact on both sides: a certain fallback
    judged = (eps < 0.25) | sure
    gn = np.linalg.norm(G, axis=1)                   # ||g_j||, [K, C]
    tau = np.einsum("kii->k", G).real
    wn = np.linalg.norm(w_t, axis=1)
    with np.errstate(all="ignore"):
        bar = (eps * gn[:, ref] + wn * (eps * gn.sum(axis=1) + C * U * np.abs(np.einsum("kii->ki", G)).sum(axis=1))) / np.abs(tau) + U * wn
    bar = np.where(fb_t | sure, 0.0, bar)            # a bin that falls back is e_ref exactly
    d = np.linalg.norm(w_dev - w_t, axis=1)
    d[~np.isfinite(d)] = np.inf
    fb_dev = np.all(w_dev == np.eye(C)[ref][None, :], axis=1)
    problems = []
    flags_differ = judged & (fb_dev != fb_t) & ~((C == 1) & ~fb_t)      # (C = 1: w = 1 = e_0 whether or not the bin fell back)
    if flags_differ.any():
        problems.append("%s: %d judged bins fall back on one side only, first bin %d" % (label, int(flags_differ.sum()), int(np.flatnonzero(flags_differ)[0])))
    over = judged & ~(d <= bar)
    rel = float(np.max(np.where(judged & (bar > 0), d / np.where(bar > 0, bar, 1.0), 0.0)))
    if over.any():
        k = int(np.flatnonzero(over)[0])
        problems.append("%s: bin %d: ||w - teacher|| = %.3e for the bar %.3e (cond %.3e); %d bins over" % (label, k, d[k], bar[k], cond[k], int(over.sum())))
    return Verdict(ok=not problems, message="; ".join(problems), rel=rel, fallback=fb_t, judged=judged, cond=cond)


def check_filter(label, y_dev, lm_dev, ph_dev, X_dev, w_dev, gain=None):
    """The device's y, lm, ph [T, 201] against the double sum of its own X and w, and the rows against its own y."""
    Xd = X_dev.astype(np.complex128)
    C = Xd.shape[0]
    y = mvdr.apply(Xd, w_dev)
    sabs = np.einsum("kc,ctk->tk", np.abs(w_dev), np.abs(Xd))
    bar = 2.0 ** -24 * np.abs(y) + 8.0 * C * U * sabs + 2.0 ** -149
    d = np.abs(y_dev.astype(np.complex128) - y)
    d[~np.isfinite(d)] = np.inf
    problems = []
    rel = float((d / bar).max())
    if rel > 1.0:
        t, k = np.unravel_index(int((d / bar).argmax()), d.shape)
        problems.append("%s: y at frame %d bin %d off by %.3e for the bar %.3e" % (label, t, k, d[t, k], bar[t, k]))
    yd = y_dev.astype(np.complex128)
    want_lm = np.log(np.maximum(np.abs(yd), mvdr.FLOOR))
    tol = 2.0 ** -22 * (1.0 + np.abs(want_lm))
    got_lm = lm_dev.astype(np.float64)
    if gain is not None:                               # one float32 addition more
        want_lm = want_lm + gain.astype(np.float64)
        tol = tol + 2.0 ** -23 * (np.abs(want_lm) + np.abs(gain))
    dl = np.abs(got_lm - want_lm)
    dl[~np.isfinite(dl)] = np.inf
    rel_lm = float((dl / tol).max())
    if rel_lm > 1.0:
        t, k = np.unravel_index(int((dl / tol).argmax()), dl.shape)
        problems.append("%s: lm at frame %d bin %d off by %.3e for %.3e" % (label, t, k, dl[t, k], tol[t, k]))
    normal = np.maximum(np.abs(yd.real), np.abs(yd.imag)) >= float(np.finfo(np.float32).tiny)
    dp = np.abs(np.angle(np.exp(1j * (ph_dev.astype(np.float64) - np.angle(yd)))))
    dp[~np.isfinite(dp)] = np.inf
    dp = np.where(normal, dp, 0.0)
    rel_ph = float(dp.max() / 4e-7)
    if rel_ph > 1.0:
        t, k = np.unravel_index(int(dp.argmax()), dp.shape)
        problems.append("%s: ph at frame %d bin %d off by %.3e rad" % (label, t, k, dp[t, k]))
    if not (np.abs(ph_dev) <= np.float32(np.pi)).all():
        problems.append("%s: a phase outside [-pi, pi]" % label)
    return Verdict(ok=not problems, message="; ".join(problems), rel=rel, rel_lm=rel_lm, rel_ph=rel_ph)


def record_bars(rec, X_dev, y_dev, ref):
    """(want energy_ref, want energy_out, relative tolerance): sums of T x 201 non-negative terms, each one rounding, in
    some fixed order: (T 201 + 2) u of the sum."""
    Xd, yd = X_dev.astype(np.complex128), y_dev.astype(np.complex128)
    n = Xd.shape[1] * BINS
    return float((np.abs(Xd[ref]) ** 2).sum()), float((np.abs(yd) ** 2).sum()), (n + 2) * U * 2
