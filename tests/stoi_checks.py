"""What tests/test_stoi_host.py and tests/test_gpu_stoi.py share: the clips (all at 10 kHz), the float64 bar and the
planted faults.

The bar.  The reference (nhans_amd.score.stoi_reference) forms every sum with math.fsum and transforms with np.fft.rfft;
the device (stoi.hip) adds in fixed orders of its own and transforms with a radix-8 transform in double.  U = 2^-53.

  * A sample of an analysis frame, a = w (w x + w' x'), carries three products, one sum and the rounding of the window
    table on either side: 6 U relative to its terms.  The two transforms -- the reference's and the device's -- each have
    a norm-wise error of order log2(512) U |X|_2 with |X|_2 = sqrt(512) |a|_2 (Parseval), and whatever of it falls into
    a band is at most all of it.  So a band value B = sqrt(sum |X(k)|^2) is off by at most
        K_T U sqrt(512) |a|_2,  K_T = 2 log2(512) + 6 = 24,
    plus (width + 4) U B for its sum of `width` terms added in any order, the squares and the root.
  * v -> (v - mean v) / (|v - mean v| + eps) over n values with elementwise errors dv:  the centred values are off by
    dc = dv + mean(dv) + (n + 2) U mean|v| + U |c|, the norm by at most |dc|_2, the result u by
        du = dc / |c| + |u| |dc|_2 / |c| + (n / 2 + 4) U |u|
    -- the first-order sensitivity |v| / |v - mean v| the issue names, taken element by element from the reference's own
    values.  A row that is constant (|c| = 0) has no finite bar.
  * STOI, per band: a = |x| / (|y| + eps) is off by da = a (|dx|_2 / |x| + |dy|_2 / |y| + (n + 6) U); y' = min(a y, c x) is
    1-Lipschitz in both arguments: dy' = max(a dy + |y| da, c dx) + 2 U |y'| (c itself is one rounding of 1 + 10^0.75 on
    either side, inside the 2 U).  The correlation sum_q x^ y'^ is off by sum (|x^| dy'^ + |y'^| dx^) + (n + 2) U sum |x^ y'^|,
    d_s by the mean of that over the bands plus (15 + 2) U mean |corr_j|.
  * Extended STOI: the rule above along the rows, then along the columns with the rows' du as dv; e_s is off by
    sum (|x~| dy~ + |y~| dx~) / 30 + (450 + 2) U sum |x~ y~| / 30.
  * The clip's mean over S segments adds (S + 1) U mean |value|.

C_BAR = 2 is the stated constant on all of it, for the second-order terms dropped above.  It is not tuned: the worst
measured ratio to the bar is in profiles/stoi/README.md, and a ratio above one half would be a defect to find.

Two conditions keep the bar honest; `conditions` asserts both on the reference alone, for every clip a test holds to it:
  1. the silent-frame margin: every frame's P_m / (P_max 1e-4) is at least MARGIN = 1e-6 away from 1, so the decision
     cannot flip on a rounding (P_m itself is off by (256 + 4) U relative, eleven orders of magnitude less);
  2. the cap: the bars on stoi and estoi are below CAP = 1e-9, so a lax derivation cannot hide a real error.

Planted faults (test_stoi_host.py): each must leave the bar by orders of magnitude, so the bar is known to see them."""
import math

import numpy as np

from nhans_amd import score

U = 2.0 ** -53
C_BAR = 2.0
K_T = 2.0 * math.log2(score.STOI_FFT) + 6.0
MARGIN = 1e-6
CAP = 1e-9
N = score.STOI_SEGMENT
LENGTHS = [0, 1, 256, 257, 384, 385, 4096, 4097, 4224, 4225, 4226, 7001]
COMPACTION = ("none", "first", "last", "every_second", "run_leaves_31", "run_leaves_30")
COMPACTION_N = 8000                                         # 61 frames


# ---- clips ----------------------------------------------------------------------------------------
def clip(n, seed):
    """-> (estimate, target) float32 [n] at 10 kHz: a target of speech-like level and an estimate 5 - 6 dB away from it"""
    rng = np.random.default_rng(2000 + seed)
    t = (0.3 * rng.standard_normal(n)).astype(np.float32)
    e = (0.9 * t + 0.15 * rng.standard_normal(n)).astype(np.float32)
    return e, t


def length_clips():
    return [clip(n, i) for i, n in enumerate(LENGTHS)]


def compaction_clip(kind):
    """8,000 samples = 61 frames (8,450 = 65 for "every_second", so that 32 frames and two segments are left) whose target is scaled by 1e-4 (80 dB down, the range is 40) over chosen samples.  A frame
    is silent when both of its 128-sample halves are scaled; a frame with one scaled half keeps about half its power.
    "every_second": frames overlap by half, so no frame between two wholly scaled ones could be loud -- instead the
    target is loud only on the 8 samples around the centre of every odd frame, which lie where the window of the even
    frames is below 1e-2 (its square below 1e-4 of the odd frames')."""
    n = 8450 if kind == "every_second" else COMPACTION_N
    e, t = clip(n, 100 + COMPACTION.index(kind))
    M = score.stoi_num_frames(n)
    low = np.zeros(n, bool)
    if kind == "first":
        low[:256] = True
    elif kind == "last":
        low[128 * (M - 1):128 * (M - 1) + 256] = True
    elif kind == "every_second":
        low[:] = True
        for m in range(1, M, 2):
            low[128 * m + 124:128 * m + 132] = False
    elif kind == "run_leaves_31":
        low[128 * 10:128 * (10 + 31)] = True                # frames 10 ... 39: 30 silent
    elif kind == "run_leaves_30":
        low[128 * 10:128 * (10 + 32)] = True                # frames 10 ... 40: 31 silent
    t = np.where(low, t * np.float32(1e-4), t).astype(np.float32)
    return e, t


def clipped_clip():
    """every twelfth frame the estimate is 40 times louder and the target 10 dB quieter (a y is at most sqrt(30) times the
    band's root mean square of x, so the clipping at 6.6 x only acts where x is below its average): y' is clipped there"""
    e, t = clip(COMPACTION_N, 120)
    for m in range(3, 60, 12):
        e[128 * m:128 * m + 256] *= np.float32(40.0)
        t[128 * m:128 * m + 256] *= np.float32(0.3)
    return e, t


def opposed_clip():
    """target and estimate share a carrier and carry opposite envelopes over blocks of 512 samples: stoi is negative"""
    rng = np.random.default_rng(2200)
    c = 0.3 * rng.standard_normal(COMPACTION_N)
    g = np.where((np.arange(COMPACTION_N) // 512) % 2 == 0, 1.0, 0.2)
    return (c * (1.2 - g)).astype(np.float32), (c * g).astype(np.float32)


# ---- the bar --------------------------------------------------------------------------------------
def _steps(e, t):
    """the reference's intermediate values: (windowed target frames, keep mask, powers, analysis frames and band tensors
    of target and estimate)"""
    n = min(len(e), len(t))
    e64, t64 = np.asarray(e[:n], np.float32).astype(np.float64), np.asarray(t[:n], np.float32).astype(np.float64)
    w = score.stoi_window()
    ft, fe = score.stoi_frames(t64, w), score.stoi_frames(e64, w)
    keep, p = score.stoi_keep(ft)
    ax, ay = score.stoi_frames(score.stoi_rejoin(ft[keep]), w), score.stoi_frames(score.stoi_rejoin(fe[keep]), w)
    return keep, p, ax, ay, score.stoi_bands_of(ax), score.stoi_bands_of(ay)


def margin(t):
    """min over the target's frames of |P_m / (P_max 1e-4) - 1| (inf without a frame or with P_max == 0)"""
    w = score.stoi_window()
    _, p = score.stoi_keep(score.stoi_frames(np.asarray(t, np.float32).astype(np.float64), w))
    if not len(p) or p.max() == 0.0:
        return math.inf
    return float(np.min(np.abs(p / (p.max() * score.STOI_RANGE) - 1.0)))


def band_errors(a, B):
    """analysis frames [Mf, 256], their band values [Mf, 15] -> elementwise error bounds [Mf, 15]"""
    norm = np.array([math.sqrt(math.fsum(f * f)) for f in a]).reshape(len(a), 1)
    width = np.array([hi - lo for lo, hi in score.STOI_BANDS], dtype=np.float64)[None, :]
    return K_T * U * math.sqrt(score.STOI_FFT) * norm + (width + 4.0) * U * B


def unit_errors(v, dv):
    """-> (u = (v - mean) / (|v - mean| + eps), elementwise bound on its error)"""
    n = len(v)
    c = v - math.fsum(v) / n
    nc = math.sqrt(math.fsum(c * c))
    u = c / (nc + score.STOI_EPS)
    if nc == 0.0:
        return u, np.full(n, math.inf)
    dc = dv + dv.mean() + (n + 2) * U * np.abs(v).mean() + U * np.abs(c)
    return u, dc / nc + np.abs(u) * math.sqrt(float(np.sum(dc * dc))) / nc + (n / 2.0 + 4.0) * U * np.abs(u)


def segment_bars(X, Y, dX, dY):
    """[30, 15] band values and their error bounds -> (bar on d_s, bar on e_s), C_BAR included"""
    n, nb = X.shape
    dd = 0.0
    corr_abs = 0.0
    Rx, Ry, dRx, dRy = (np.empty((n, nb)) for _ in range(4))
    for j in range(nb):
        x, y, dx, dy = X[:, j], Y[:, j], dX[:, j], dY[:, j]
        nx, ny = math.sqrt(math.fsum(x * x)), math.sqrt(math.fsum(y * y))
        a = nx / (ny + score.STOI_EPS)
        with np.errstate(divide="ignore", invalid="ignore"):
            da = a * (np.linalg.norm(dx) / nx + np.linalg.norm(dy) / ny + (n + 6) * U) if nx > 0 and ny > 0 else math.inf
        yp = np.minimum(a * y, score.STOI_CLIP * x)
        dyp = np.maximum(a * dy + np.abs(y) * da, score.STOI_CLIP * dx) + 2.0 * U * np.abs(yp)
        ux, dux = unit_errors(x, dx)
        up, dup = unit_errors(yp, dyp)
        dd += float(np.sum(np.abs(ux) * dup + np.abs(up) * dux)) + (n + 2) * U * float(np.sum(np.abs(ux * up)))
        corr_abs += abs(math.fsum(ux * up))
        Rx[:, j], dRx[:, j] = ux, dux
        Ry[:, j], dRy[:, j] = unit_errors(y, dy)
    dd = dd / nb + (nb + 2) * U * corr_abs / nb
    de = 0.0
    tot = 0.0
    for q in range(n):
        cx, dcx = unit_errors(Rx[q], dRx[q])
        cy, dcy = unit_errors(Ry[q], dRy[q])
        de += float(np.sum(np.abs(cx) * dcy + np.abs(cy) * dcx))
        tot += float(np.sum(np.abs(cx * cy)))
    de = de / n + (n * nb + 2) * U * tot / n
    return C_BAR * dd, C_BAR * de


def conditions(ref, bar, t):
    """the two conditions of the docstring, on the reference alone"""
    m = margin(t[:ref["n"]])
    assert m >= MARGIN, "silent-frame margin %.3e" % m
    if ref["segments"]:
        assert bar["stoi"] < CAP and bar["estoi"] < CAP, bar


def stoi_bar(e, t):
    """-> (reference record with "per_segment", {"stoi", "estoi": absolute bar}, per-segment bars [S, 2]); asserts the two
    conditions"""
    ref = score.stoi_reference(e, t, per_segment=True)
    _, _, ax, ay, X, Y = _steps(e, t)
    dX, dY = band_errors(ax, X), band_errors(ay, Y)
    S = ref["segments"]
    per = np.array([segment_bars(X[s:s + N], Y[s:s + N], dX[s:s + N], dY[s:s + N]) for s in range(S)], dtype=np.float64).reshape(S, 2)
    bar = {}
    for i, k in enumerate(("stoi", "estoi")):
        bar[k] = float(per[:, i].mean()) + C_BAR * (S + 1) * U * float(np.abs(ref["per_segment"][:, i]).mean()) if S else 0.0
    conditions(ref, bar, np.asarray(t))
    return ref, bar, per


def ratio(got, ref, bar):
    """|got - ref| / bar; values that are not finite must be THE SAME non-finite value (ratio 0), else inf."""
    got, ref = float(got), float(ref)
    if not (math.isfinite(got) and math.isfinite(ref)):
        same = (math.isnan(got) and math.isnan(ref)) or got == ref
        return 0.0 if same else math.inf
    if got == ref:
        return 0.0
    return abs(got - ref) / bar if bar > 0 else math.inf


def stoi_ratios(got, e, t, counts=True):
    """got: dict by score.STOI_FIELDS (+ optional "per_segment") -> {figure: ratio to the bar}; the counts must be equal"""
    ref, bar, per = stoi_bar(e, t)
    if counts:
        for k in ("n", "frames", "frames_kept", "segments"):
            assert int(got[k]) == ref[k], (k, got[k], ref[k])
    out = {k: ratio(got[k], ref[k], bar[k]) for k in ("stoi", "estoi")}
    if "per_segment" in got and counts:
        assert np.shape(got["per_segment"]) == (ref["segments"], 2)
        out["per_segment"] = max([ratio(g, r, b) for g, r, b in zip(np.ravel(got["per_segment"]), np.ravel(ref["per_segment"]),
                                                                  np.ravel(per))], default=0.0)
    return out


# ---- planted faults: the reference's steps put together wrongly ------------------------------------
def _figures(X, Y, segment=score.stoi_segment, esegment=score.estoi_segment):
    S = max(len(X) - N + 1, 0)
    d = [segment(X[s:s + N], Y[s:s + N]) for s in range(S)]
    e = [esegment(X[s:s + N], Y[s:s + N]) for s in range(S)]
    return {"segments": S, "stoi": math.fsum(d) / S if S else math.nan, "estoi": math.fsum(e) / S if S else math.nan}


def _faulty(e, t, drop_last=False, mask_from_estimate=False, second_window=True, bands=score.STOI_BANDS, **kw):
    n = min(len(e), len(t))
    e64, t64 = np.asarray(e[:n], np.float32).astype(np.float64), np.asarray(t[:n], np.float32).astype(np.float64)
    w = score.stoi_window()
    ft, fe = score.stoi_frames(t64, w), score.stoi_frames(e64, w)
    keep, _ = score.stoi_keep(fe if mask_from_estimate else ft)
    if drop_last:
        keep[np.flatnonzero(keep)[-1]] = False
    w2 = w if second_window else np.ones_like(w)
    X = score.stoi_bands_of(score.stoi_frames(score.stoi_rejoin(ft[keep]), w2), bands)
    Y = score.stoi_bands_of(score.stoi_frames(score.stoi_rejoin(fe[keep]), w2), bands)
    return _figures(X, Y, **kw)


def fault_last_kept_frame_dropped(e, t):
    return _faulty(e, t, drop_last=True)


def fault_mask_from_estimate(e, t):
    return _faulty(e, t, mask_from_estimate=True)


def fault_window_once(e, t):
    return _faulty(e, t, second_window=False)


def fault_band_edge_off_by_one(e, t):
    bands = list(score.STOI_BANDS)
    bands[7] = (bands[7][0], bands[7][1] + 1)
    return _faulty(e, t, bands=tuple(bands))


def fault_clip_factor(e, t):
    return _faulty(e, t, segment=lambda X, Y: score.stoi_segment(X, Y, clip=10.0 ** (15.0 / 20.0)))


def fault_columns_before_rows(e, t):
    return _faulty(e, t, esegment=lambda X, Y: score.estoi_segment(X.T, Y.T) * X.shape[1] / X.shape[0])
