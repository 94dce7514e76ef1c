"""Shared pieces of the STFT / inverse STFT domain tests (tests/test_gpu_stft_domain.py on the device,
tests/test_stft_checks_host.py for the CPU half): the signal classes, the float64 references (oracle/nhans_oracle.py), the
float32 CPU restatement of both directions, the bar, a comparison that says WHERE a result is wrong -- (class, clip, frame,
bin) -- and the faults planted in the restatement to show that the comparison catches what it is for.

The yardstick of every bar is the float32 CPU restatement against float64 -- what any correct float32 implementation may
differ by --, never the device's own output.

Analysis, per FRAME, in the linear complex domain  z = (exp(lm) - 1e-5) * exp(1j * ph)  against X (float64 arithmetic):

    err(frame) = max_k |z - X|          bar(frame) = K * ratio(class) * max_k|X| + A

ratio(class) is the largest  max(err - A, 0) / max_k|X|  of the restatement over the frames of the class whose maximum is
at least TINY.  A = 1e-10 is the absolute term: ten times what the float32 rounding of ln 1e-5 is worth after exp (half an
ulp at 11.5 is 4.8e-7, times 1e-5).  That rounding is absolute -- it does not shrink with the frame --, so a frame at 1e-8
has 5e-4 of its maximum of it: A carries it in the bar, and it is taken out of the ratio so that a class that decays
through such frames (the fade) is not judged, nor capped, by them; on every other class this only makes the bar smaller.
Frames whose maximum is below TINY = 1e-30 get the absolute term alone.  The cap -- a condition, not a measurement -- is
K * ratio < 1e-5, the per-clip bar of the older tests applied to the frame.

Inverse, per CLIP:  bar = K * max|cpu32 - f64| + F * max|f64|,  capped by 8.6e-5 * max|f64| (the absolute 2e-5 of
test_istft_matches_oracle_and_is_linear_in_magnitude over the peak 0.2314 of its first clip's reference).  profiles/stft_domain/README.md holds
the measurement F comes from.
"""
import numpy as np
import torch

import nhans_amd  # noqa: F401
import oracle.nhans_oracle as O

WIN, HOP, BINS = O.WIN, O.HOP, O.BINS
FRAMES = 30
SAMPLES = WIN + HOP * (FRAMES - 1)          # 4,960
FLOOR = float(np.log(1e-5))
STFT_RUN = 23                               # frames per run of the analysis kernel
ISTFT_RUN = 22                              # output hops per run of the inverse kernel (frames h0 - 2 .. h0 + 21)

# ---- the bar -----------------------------------------------------------------------------------------------------
K = 4.0                 # tests/layer_checks.py's K, fixed before the first run
A = 1e-10
TINY = 1e-30
CAP_ANALYSIS = 1e-5
CAP_INVERSE = 8.6e-5
PHASE_TOL = 1e-4        # wrapped, where |X| > LOUD * max_k|X| of the frame
LOUD = 1e-2
FLOOR_TOL = 1e-6        # |lm - ln 1e-5| where |X| < SILENT in a frame whose max_k|X| < QUIET_FRAME
SILENT = 1e-12
# (a silent bin of a frame that has energy elsewhere holds that frame's float32 rounding -- 3e-7 of its maximum in any
# float32 transform, 6e-5 beside DC 1.0's bin 0 -- and log(. + 1e-5) shows it; such bins are judged by the frame's bar.  Below
# 1e-6 that rounding is under 1e-12 and moves lm by less than 1e-7.)
QUIET_FRAME = 1e-6
# The device's share of max|f64| on top of K x err_cpu32 in the inverse direction: none is needed -- on the MI355X the worst
# class with phases inside [-pi, pi] sits at 1.30 x err_cpu32 (profiles/stft_domain/README.md).
F_INVERSE = 0.0


# ---- signal classes (analysis) -----------------------------------------------------------------------------------
def _noise(seed, n=SAMPLES):
    return np.random.default_rng(seed).standard_normal(n)


def analysis_classes():
    """[(name, float32 samples)]: one clip of 30 frames per class, fixed seeds."""
    n = np.arange(SAMPLES, dtype=np.float64)
    g = _noise(1001)
    imp = np.zeros(SAMPLES)
    imp[[0, 159, 160, 399, 400, 1000]] = 1.0
    step = np.where(n < 2000, 1.0, 1e-4)
    cls = [
        ("1 noise sigma 1", g),
        ("2 noise int16 scale", np.clip(np.rint(g * 8000.0), -32768, 32768)),
        ("3 noise 1e-6", g * 1e-6),
        ("4 dc", np.ones(SAMPLES)),
        ("5 impulses", imp),
        ("6 exact-bin cosines 1 37 100 199", sum(np.cos(2 * np.pi * k * n / WIN) for k in (1, 37, 100, 199))),
        ("7 nyquist", np.where(n % 2 == 0, 1.0, -1.0)),
        ("8 off-bin cosine 37.37", np.cos(2 * np.pi * 37.37 * n / WIN + 0.3)),
        ("9 fade through the denormals", _noise(1009) * np.exp(-n / SAMPLES * np.log(1e44))),
        ("10 loud then 1e-4", _noise(1010) * step),
        ("11 zeros", np.zeros(SAMPLES)),
    ]
    return [(name, np.asarray(x, dtype=np.float32)) for name, x in cls]


# Clip i of the frame-count launch has i + 1 frames and (TAIL_MULT * i) % 160 untrimmed samples after them.  The
# multiplier 37 reaches the remainder 159 only at i = 147; 137 has 0 at i = 0 and 159 at i = 7.
COUNT_CLIPS = 50
TAIL_MULT = 137


def count_tails():
    return [(TAIL_MULT * i) % HOP for i in range(COUNT_CLIPS)]


def count_clips():
    """50 clips of sigma-1 noise, T = 1 .. 50 frames, tails untrimmed."""
    return [_noise(2000 + i, WIN + HOP * i + r).astype(np.float32) for i, r in enumerate(count_tails())]


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


# ---- float32 CPU restatement, analysis ---------------------------------------------------------------------------
# Bins the analysis kernel writes as conjugates of bins 400 - k of its 20 x 20 transform (rows k1 = 1 .. 9, k2 >= 10)
MIRRORED = np.array([b for b in range(BINS) if (WIN - b) // 20 >= 10 and 1 <= (WIN - b) % 20 <= 9 and b > 0])
ANALYSIS_FAULTS = ("mirror_swap", "conj_dropped", "leak", "run_end_zeroed")
LEAK_FROM = 12          # class 10: the last frame with loud samples; frame 13 is the first all-quiet one


def _frames32(wav):
    wav = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
    t = 1 + (len(wav) - WIN) // HOP if len(wav) >= WIN else 0
    idx = torch.arange(WIN)[None, :] + HOP * torch.arange(t)[:, None]
    win = torch.from_numpy(O.hann_periodic().astype(np.float32))
    return wav[idx] * win[None, :]


def cpu32_features(wav, fault=None):
    """torch.fft.rfft on float32 windowed frames, float32(log(|X| + 1e-5)), float32(angle): [T,201] float32 each.
    fault: one of ANALYSIS_FAULTS, planted the way the kernel could get it wrong."""
    X = torch.fft.rfft(_frames32(wav), n=WIN, dim=1)                 # complex64
    if fault == "leak":                                              # 1e-6 of frame LEAK_FROM lands in its neighbour
        X = X.clone()
        X[LEAK_FROM + 1] += np.float32(1e-6) * X[LEAK_FROM]
    lm = torch.log(X.abs() + np.float32(1e-5)).numpy()
    ph = torch.angle(X).numpy()
    assert lm.dtype == np.float32 and ph.dtype == np.float32
    if fault == "mirror_swap":
        # full-transform bin 363 = 3 + 20 * 18 is written as bin 37; taken one k2 off, it trades places with the mirror
        # of 343 = 3 + 20 * 17, bin 57
        lm[:, [37, 57]] = lm[:, [57, 37]]
        ph[:, [37, 57]] = ph[:, [57, 37]]
    elif fault == "conj_dropped":
        ph[:, MIRRORED] = -ph[:, MIRRORED]
    elif fault == "run_end_zeroed":
        lm[STFT_RUN - 1] = np.float32(FLOOR)
        ph[STFT_RUN - 1] = 0.0
    return lm, ph


def linear(lm, ph):
    lm, ph = np.asarray(lm, dtype=np.float64), np.asarray(ph, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.exp(lm) - 1e-5) * np.exp(1j * ph)


def frame_errors(lm, ph, X):
    """(err [T], max_k|X| [T], |z - X| [T,201]) in float64; non-finite entries count as inf."""
    d = np.abs(linear(lm, ph) - X)
    d[~np.isfinite(d)] = np.inf
    return d.max(axis=1), np.abs(X).max(axis=1), d


_ratios = {}


def yardstick_ratio(key, wavs):
    """ratio(class) of the module docstring over the clips `wavs` of one class; kept per key."""
    if key not in _ratios:
        r = 0.0
        for w in wavs:
            X = O.stft(w)
            err, mx, _ = frame_errors(*cpu32_features(w), X)
            ok = mx >= TINY
            if ok.any():
                r = max(r, float((np.maximum(err[ok] - A, 0.0) / mx[ok]).max()))
        _ratios[key] = r
    return _ratios[key]


class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def check_analysis(label, clip, lm, ph, wav, ratio, frames=None):
    """lm, ph ([T,201] float32; ph may be None) as features of clip `wav` of class `label` against the float64 oracle, every
    frame and bin.  frames: the rows are frames[0] .. of the clip (default: all).  Verdict: ok, message, worst =
    (frame, bin) of the largest err / bar, rel = largest max(err - A, 0) / max_k|X| (the device's figure beside `ratio`)."""
    X = O.stft(wav)
    if frames is not None:
        X = X[frames]
    lm = np.asarray(lm)
    problems = []
    where = lambda f, k: "class %s, clip %d, frame %d, bin %d" % (label, clip, f if frames is None else frames[f], k)
    if lm.shape != X.shape or lm.dtype != np.float32:
        return Verdict(ok=False, message="class %s, clip %d: log-magnitudes %s %s for %s frames x bins" % (
            label, clip, lm.shape, lm.dtype, X.shape), worst=None, rel=np.inf)
    if not K * ratio < CAP_ANALYSIS:
        problems.append("the bar %g x %.3e is not below the cap %g of the frame's maximum" % (K, ratio, CAP_ANALYSIS))
    mag = np.abs(X)
    bad = ~np.isfinite(lm)
    if bad.any():
        f, k = np.argwhere(bad)[0]
        problems.append("log-magnitude %r at %s (%d non-finite)" % (float(lm[f, k]), where(f, k), int(bad.sum())))
    fl = np.abs(lm.astype(np.float64) - FLOOR)
    fl[~np.isfinite(fl)] = np.inf
    fl = np.where((mag < SILENT) & (mag.max(axis=1, keepdims=True) < QUIET_FRAME), fl, 0.0)
    if fl.size and not fl.max() < FLOOR_TOL:
        f, k = np.unravel_index(int(fl.argmax()), fl.shape)
        problems.append("|lm - ln 1e-5| = %.3e at %s, where |X| = %.3e" % (fl[f, k], where(f, k), mag[f, k]))
    phz = np.zeros_like(lm) if ph is None else np.asarray(ph)
    if ph is not None:
        bad = ~(np.abs(phz) <= np.float32(np.pi))                    # NaN fails; float32(pi) is the largest |angle| stored
        if bad.any():
            f, k = np.argwhere(bad)[0]
            problems.append("phase %r at %s (%d outside [-pi, pi] or non-finite; |X| = %.3e)" % (
                float(phz[f, k]), where(f, k), int(bad.sum()), mag[f, k]))
    err, mx, d = frame_errors(lm, phz if ph is not None else np.angle(X), X)
    bar = np.where(mx >= TINY, K * ratio * mx, 0.0) + A
    worst = (0, 0)
    rel = 0.0
    if len(err):
        f = int(np.argmax(err / bar))
        worst = (f if frames is None else frames[f], int(d[f].argmax()))
        ok = mx >= TINY
        rel = float((np.maximum(err[ok] - A, 0.0) / mx[ok]).max()) if ok.any() else 0.0
        if not err[f] <= bar[f]:
            k = int(d[f].argmax())
            problems.append("|z - X| = %.3e above the bar %.3e (= %g x %.3e x max_k|X| %.3e + %g) at %s: z %r, X %r; %d of %d "
                            "frames above their bar" % (err[f], bar[f], K, ratio, mx[f], A, where(f, k),
                                                        complex(linear(lm[f, k], phz[f, k])) if ph is not None else None,
                                                        complex(X[f, k]), int((err > bar).sum()), len(err)))
    if ph is not None:
        dp = np.abs(np.angle(np.exp(1j * (phz.astype(np.float64) - np.angle(X)))))
        dp[~np.isfinite(dp)] = np.inf
        dp = np.where((mag > LOUD * mx[:, None]) & (mx[:, None] >= TINY), dp, 0.0)
        if dp.size and not dp.max() < PHASE_TOL:
            f, k = np.unravel_index(int(dp.argmax()), dp.shape)
            problems.append("phase off by %.3e rad at %s: %r for %r" % (dp[f, k], where(f, k), float(phz[f, k]),
                                                                        float(np.angle(X[f, k]))))
    return Verdict(ok=not problems, message="; ".join(problems), worst=worst, rel=rel, ratio=ratio,
                   err=err, bar=bar, label=label, clip=clip)


# ---- inverse ------------------------------------------------------------------------------------------------------
def inverse_classes(ph1):
    """[(name, lm [30,201] float32, ph [30,201] float32)] -- ph1: phases of analysis class 1 (the device's own on the
    device, the restatement's on the host)."""
    ph1 = np.asarray(ph1, dtype=np.float32)
    assert ph1.shape == (FRAMES, BINS)
    rng = np.random.default_rng(3001)
    u = lambda lo, hi: rng.uniform(lo, hi, (FRAMES, BINS)).astype(np.float32)
    alt = lambda loud: np.where((np.arange(FRAMES) % 2 == loud)[:, None], np.float32(6.0), np.float32(FLOOR)) * np.ones(
        (1, BINS), np.float32)
    third = np.repeat(np.array([-np.pi, 0.0, np.pi], dtype=np.float32), BINS // 3)
    edge = ph1.copy()
    edge[:, 0] = rng.uniform(0.3, 3, FRAMES) * rng.choice([-1.0, 1.0], FRAMES)
    edge[:, BINS - 1] = rng.uniform(0.3, 3, FRAMES) * rng.choice([-1.0, 1.0], FRAMES)
    two_pi = np.float64(2 * np.pi)
    return [
        ("1 lm in [ln 1e-5, 0]", u(FLOOR, 0.0), ph1),
        ("2 lm in [ln 1e-5 - 20, ln 1e-5]", u(FLOOR - 20.0, FLOOR), ph1),
        ("3 lm in [0, 16]", u(0.0, 16.0), ph1),
        ("4a loud frames in the a position", alt(0).astype(np.float32), ph1),
        ("4b loud frames in the b position", alt(1).astype(np.float32), ph1),
        ("5 phases -pi 0 +pi", u(FLOOR, 0.0), np.broadcast_to(third, (FRAMES, BINS)).copy()),
        ("6 phase at bins 0 and 200", u(FLOOR, 0.0), edge),
        ("7a phases + 6 pi", u(FLOOR, 0.0), (ph1.astype(np.float64) + 3 * two_pi).astype(np.float32)),
        ("7b phases - 6 pi", u(FLOOR, 0.0), (ph1.astype(np.float64) - 3 * two_pi).astype(np.float32)),
    ]


def count_spectra():
    """50 clips with T = 1 .. 50 frames: lm uniform in [ln 1e-5, 0], phases uniform in [-pi, pi]."""
    rng = np.random.default_rng(3002)
    return [(rng.uniform(FLOOR, 0.0, (t, BINS)).astype(np.float32), rng.uniform(-np.pi, np.pi, (t, BINS)).astype(np.float32))
            for t in range(1, COUNT_CLIPS + 1)]


INVERSE_FAULTS = ("nyquist_imag",)


def cpu32_inverse(lm, ph, fault=None):
    """exp and polar in float32, torch.fft.irfft in float32, synthesis window and overlap-add in float32.
    fault "nyquist_imag": frames (2k, 2k + 1) share one complex transform Z = A + iB on the device; with the imaginary part
    of bin 200 kept, Im A[200] shows up in frame b and -Im B[200] in frame a, as (-1)^n / 400."""
    lm = torch.from_numpy(np.ascontiguousarray(lm, dtype=np.float32))
    ph = torch.from_numpy(np.ascontiguousarray(ph, dtype=np.float32))
    spec = torch.polar(torch.exp(lm), ph)                            # complex64
    fr = torch.fft.irfft(spec, n=WIN, dim=1)
    assert fr.dtype == torch.float32
    t = fr.shape[0]
    if fault == "nyquist_imag":
        alt = torch.from_numpy(np.where(np.arange(WIN) % 2 == 0, 1.0, -1.0).astype(np.float32)) / np.float32(WIN)
        im = spec[:, BINS - 1].imag
        fr = fr.clone()
        for a in range(0, t - 1, 2):
            fr[a + 1] += im[a] * alt
            fr[a] -= im[a + 1] * alt
    fr = fr * torch.from_numpy(O.istft_window().astype(np.float32))[None, :]
    out = torch.zeros((t - 1) * HOP + WIN, dtype=torch.float32)
    for i in range(t):
        out[i * HOP:i * HOP + WIN] += fr[i]
    return out.numpy()


# Phases outside [-pi, pi] (include/nhans_hip.h: accepted, at reduced accuracy).  The kernel hands the angle to v_sin / v_cos
# in revolutions, rev = a / 2 pi rounded to float32; the CPU's sinf reduces the float32 angle exactly.  At |a| = 7 pi, rev is
# in [2, 4): half an ulp of it is 2^-23 revolutions = 7.5e-7 rad, against 2^-26 revolutions inside [-pi, pi].
PHASE_SLACK_7PI = 2 * np.pi * 2.0 ** -23


def phase_sensitivity(lm):
    """The largest |d out[n] / d phase| summed over all bins: a phase error of d rad in every bin moves no output sample by
    more than d times this (bin k of frame f enters sample n as (2 / 400) exp(lm) cos(. + ph) wsyn)."""
    lm = np.asarray(lm, dtype=np.float64)
    per_frame = (2.0 / WIN) * np.exp(lm).sum(axis=1)
    out = np.zeros((lm.shape[0] - 1) * HOP + WIN)
    w = np.abs(O.istft_window())
    for i, s in enumerate(per_frame):
        out[i * HOP:i * HOP + WIN] += s * w
    return float(out.max())


def check_inverse(label, clip, out, lm, ph, f_share=None, phase_slack=0.0):
    """out (float32 samples of one clip) against recover_samples in float64.  phase_slack (rad): what the clip's phases may be
    off by per bin by contract; it enters the bar as phase_slack x phase_sensitivity(lm), a worst case worked out from the
    input alone.  Verdict: ok, message, err_hip, err_cpu32, m."""
    f_share = F_INVERSE if f_share is None else f_share
    lm, ph = np.asarray(lm), np.asarray(ph)
    ref = O.recover_samples(lm.astype(np.float64), ph.astype(np.float64))
    out = np.asarray(out)
    if out.shape != ref.shape or out.dtype != np.float32:
        return Verdict(ok=False, message="class %s, clip %d: %s %s samples for %s" % (label, clip, out.shape, out.dtype, ref.shape),
                       err_hip=np.inf, err_cpu32=0.0, m=0.0)
    err_cpu32 = float(np.abs(cpu32_inverse(lm, ph) - ref).max())
    m = float(np.abs(ref).max())
    d = np.abs(out.astype(np.float64) - ref)
    d[~np.isfinite(d)] = np.inf
    err = float(d.max())
    bar = K * err_cpu32 + f_share * m + (phase_slack * phase_sensitivity(lm) if phase_slack else 0.0)
    i = int(d.argmax())
    problems = []
    if not err <= bar:
        last = min(i // HOP, lm.shape[0] - 1)
        problems.append("max|out - f64| %.3e above the bar %.3e (%g x err_cpu32 %.3e + %g x max %.3e + phase slack) at sample %d (hop %d, "
                        "frames %d..%d of %d): %r for %r; %d samples above" % (
                            err, bar, K, err_cpu32, f_share, m, i, i // HOP, max(0, i // HOP - 2), last, lm.shape[0],
                            float(out[i]), float(ref[i]), int((d > bar).sum())))
    if not bar < CAP_INVERSE * m:
        problems.append("the bar %.3e is not below the cap %g x max = %.3e" % (bar, CAP_INVERSE, CAP_INVERSE * m))
    msg = "class %s, clip %d: %s" % (label, clip, "; ".join(problems)) if problems else ""
    return Verdict(ok=not problems, message=msg, err_hip=err, err_cpu32=err_cpu32, m=m, bar=bar, worst=i, label=label, clip=clip)
