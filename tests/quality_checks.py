"""What the tests of nhans_quality share (quality.hip; the definition: include/nhans_hip.h and score.quality_reference).

BIT FOR BIT.  `device_order_lpc` repeats the header's operation list on the host -- every fused multiply-add through the C
library's fma, which rounds once -- and holds the per-frame r[k], a[k], num, den and dc2 of nhans_quality_lpc to the bit.

WITHIN BARS.  ln, log10, pow, the transform and the means are held to score.quality_reference, whose sums are exactly
rounded.  Every bar counts roundings of u = 2^-53; none carries a constant taken from the device's output.

  r[k]     the device's chain rounds each of its <= N = 480 terms once and each partial sum once, the reference each term
           once and the sum once: |dr[k]| <= (N + 1) u sum_i |xw[i] xw[i + k]| <= (N + 1) u r[0]  (Cauchy-Schwarz).
  a        a solves the Toeplitz system of r.  Perturbing every entry of the P x P matrix by (N + 1) u r[0] perturbs it by at
           most P (N + 1) u r[0] in the 2-norm, i.e. by P (N + 1) u relative to ||R||_2 >= r[0], and the right side
           likewise: to first order ||da|| / ||a|| <= 2 cond2(R) P (N + 1) u.  Levinson-Durbin on a positive definite
           matrix is stable in the way Cholesky is (Cybenko 1980): its own roundings lose at most P^2 u cond2(R), for the
           device's recursion and for the reference's each.  C_A = 2 P (N + 1) + 4 P^2 = 16,416 (the last term twice for
           margin):   ||da||_2 <= C_A u cond2(R) ||a||_2,  cond2 of the 17 x 17 matrix, which bounds the 16 x 16 one's
           (interlacing).  Levinson-Durbin loses that much, so the LLR and CD bars carry the frame's cond2(R).
  den      q(a_t) at its minimiser: R_t a_t = (E, 0, ..., 0) and da[0] = 0, so the term linear in da is of second order
           too: |dden| <= 3 ||R_t||_2 ||da_t||^2 + F u r_t[0] ||a_t||_1^2,  F = (N + 1) + 2 (P + 1) + 2: the perturbation of
           R's entries and the 2 (P + 1) + 2 roundings a term of the double chain meets.
  num      |dnum| <= 2 ||R_t a_e||_2 ||da_e|| + ||R_t||_2 ||da_e||^2 + F u r_t[0] ||a_e||_1^2.
  llr      x = dnum / num + dden / den (asserted < 1/2, where |ln(1 + x)| <= 2 |x|): bar = 2 x + 8 u max(1, |ln(num / den)|) -- the
           quotient's rounding and a logarithm good to a few units in the last place.  The clamp is 1-Lipschitz.
  c, cd    the recursion's error is bounded term by term: dc[m] <= da + sum_k (k / m) (dc[k] |a[m - k]| + |c[k]| da +
           dc[k] da) + 2 (m + 2) u (|a[m]| + sum_k (k / m) |c[k] a[m - k]|), da = ||da||_2 for every entry.  With D = dc2:
           dD <= sum_m (2 |d_m| e_m + e_m^2) + 2 (P + 2) u D, e_m = dc_t[m] + dc_e[m]; the root is concave, so
           bar = K max(sqrt(2 (D + dD)) - sqrt(2 D), sqrt(2 D) - sqrt(2 max(D - dD, 0))) + 8 u cd, K = 10 / ln 10.
  |X_k|    every output of the transform is sum_i x_i W^(i k) formed along a tree in which a path meets three twiddle
           products (a table entry good to u, a complex product good to 3 u: 4 u each), nine levels of additions (u each)
           and at most three constant products per stage (3 u each): 12 + 9 + 9 = 30 roundings, C_F = 32.
           |dX_k| <= C_F u ||xw||_1.  The magnitude's product, fma and root are relative to the result:
           |d|X_k|| <= 2 C_F u ||xw||_1 + 4 u |X_k|  (twice the transform's term: the reference's transform has roundings
           of its own).
  X_j      |dX_j| <= sum_k W_jk d|X_k| + 2 (nz_j + 1) u X_j, nz_j the non-zero weights of the row.
  s_j      the interval of 10 log10(X^2 / (X - Y)^2) over X +- dX and (X - Y) +- (dX + dY), clamped at both ends, plus
           16 u 45 for the products, the quotient and the logarithm: bar_s = the farther end's distance from the reference.
  g_j      dg = the farther of (X +- dX)^0.2 from X^0.2, plus 8 u g.
  fw       fw = 35 - D / G, D = sum g d, d = 35 - s in [0, 45], G = sum g: dD <= sum (dg d + g bar_s + dg bar_s) + 2 (K + 2) u
           sum g d, dG <= sum dg + 2 (K + 1) u G; bar = (dD + (35 - fw) dG) / (G - dG) + 4 u 45  (G > 2 dG asserted).
  means    the mean of errors is at most the mean of the bars, plus 2 (M + 2) u max |v| for the chain.  The mean of the q
           smallest of M values is 1-Lipschitz in the largest error of a value: bar_95 = max bar + 2 (q + 4) u max |v|.

CONDITIONS ON THE REFERENCE ALONE (`conditions`): every kept frame has cond2(R) <= 1e8 for both signals; no kept frame's
unclamped LLR or CD is within twice its bar of a clamp edge and no value other than the q-th smallest within twice its
bar of it -- unless the clip is built to sit exactly there (exact=True: e == t, a scaled copy, repeating frames)."""
import ctypes
import ctypes.util
import math

import numpy as np

import nhans_amd  # noqa: F401
from nhans_amd import hip, score

U = 2.0 ** -53
N, H, P = score.QUALITY_FRAME, score.QUALITY_HOP, score.QUALITY_ORDER
C_A = 2 * P * (N + 1) + 4 * P * P
C_F = 32
F_FORM = (N + 1) + 2 * (P + 1) + 2
COND_MAX = 1e8
LT, BT = hip.QUALITY_LPC_TILE, hip.QUALITY_BAND_TILE
NAN = float("nan")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
fma = _libm.fma


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_values(a, b):
    """equal, NaN where NaN (the payload of a NaN is not part of the contract)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~np.isnan(a)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


# ---- the header's operation list on the host ---------------------------------------------------------
def _pos_finite(v):
    return v > 0.0 and math.isfinite(v)


def _chain_autocorr(xw):
    r = []
    for k in range(P + 1):
        acc = 0.0
        for i in range(N - k):
            acc = fma(xw[i], xw[i + k], acc)
        r.append(acc)
    return r


def _levinson(r):
    a = [1.0] + [0.0] * P
    good, E = r[0] != 0.0, r[0]
    m = 1
    while m <= P and good:
        acc = r[m]
        for j in range(1, m):
            acc = fma(a[j], r[m - j], acc)
        k = -(acc / E)
        new = [fma(k, a[m - j], a[j]) for j in range(1, m)]
        a[1:m] = new
        a[m] = k
        E = E * fma(-k, k, 1.0)
        good = _pos_finite(E)
        m += 1
    if not good:
        return [1.0] + [NAN] * P, [0.0] + [NAN] * P, False
    c = [0.0] * (P + 1)
    for m in range(1, P + 1):
        s = 0.0
        for k in range(1, m):
            s = fma((float(k) / float(m)) * c[k], a[m - k], s)
        c[m] = (-a[m]) - s
    return a, c, True


def _form(a, rt):
    q = 0.0
    for i in range(P + 1):
        row = 0.0
        for j in range(P + 1):
            row = fma(rt[abs(i - j)], a[j], row)
        q = fma(a[i], row, q)
    return q


def device_order_lpc(e, t, frames=None):
    """The rows nhans_quality_lpc writes for estimate e against target t (float32), float64 [M, 72], by the header's
    operation list; frames: only these rows are worked (the others are NaN)."""
    n = min(len(e), len(t))
    w = score.quality_window()
    x = [np.asarray(s[:n], dtype=np.float32).astype(np.float64) for s in (t, e)]
    M = score.quality_num_frames(n)
    out = np.full((M, hip.QUALITY_LPC_FIELDS), NAN)
    for f in (range(M) if frames is None else frames):
        r, a, c = [], [], []
        for sg in (0, 1):
            xw = (x[sg][H * f:H * f + N] * w).tolist()
            r.append(_chain_autocorr(xw))
            aa, cc, _ = _levinson(r[sg])
            a.append(aa)
            c.append(cc)
        den, num = _form(a[0], r[0]), _form(a[1], r[0])
        dc2 = 0.0
        for m in range(1, P + 1):
            d = c[0][m] - c[1][m]
            dc2 = fma(d, d, dc2)
        out[f] = r[0] + r[1] + a[0] + a[1] + [num, den, dc2, 0.0]
    return out


def lpc_values(row):
    """(llr_f, cd_f) the device derives from a row of nhans_quality_lpc, up to its ln: for the skip rule"""
    num, den, dc2 = row[4 * (P + 1):4 * (P + 1) + 3]
    return _pos_finite(num) and _pos_finite(den) and not np.isnan(row[2 * (P + 1):4 * (P + 1)]).any()


# ---- the bars ---------------------------------------------------------------------------------------
def _cep_bar(a, c, da):
    dc = np.zeros(P + 1)
    for m in range(1, P + 1):
        acc, mag = da, abs(a[m])
        for k in range(1, m):
            acc += (k / m) * (dc[k] * abs(a[m - k]) + abs(c[k]) * da + dc[k] * da)
            mag += (k / m) * abs(c[k] * a[m - k])
        dc[m] = acc + 2 * (m + 2) * U * mag
    return dc


def lpc_bars(d):
    """d: a kept frame's dict of score.quality_lpc_frame -> dict: cond_t, cond_e, r (the bar of every r[k], [2]), llr, cd,
    and the unclamped values llr_raw, cd_raw"""
    Rt, Re = score.quality_toeplitz(d["r_t"]), score.quality_toeplitz(d["r_e"])
    ct, ce = float(np.linalg.cond(Rt)), float(np.linalg.cond(Re))
    at, ae = d["a_t"], d["a_e"]
    da_t, da_e = C_A * U * ct * np.linalg.norm(at), C_A * U * ce * np.linalg.norm(ae)
    nR = float(np.linalg.norm(Rt, 2))
    rnd = F_FORM * U * d["r_t"][0]
    dnum = 2 * np.linalg.norm(Rt @ ae) * da_e + nR * da_e ** 2 + rnd * np.abs(ae).sum() ** 2
    dden = 3 * nR * da_t ** 2 + rnd * np.abs(at).sum() ** 2
    x = dnum / d["num"] + dden / d["den"]
    raw = math.log(d["num"] / d["den"])
    llr = 2 * x + 8 * U * max(1.0, abs(raw))
    c_t, c_e = score.quality_cepstrum(at), score.quality_cepstrum(ae)
    em = _cep_bar(at, c_t, da_t) + _cep_bar(ae, c_e, da_e)
    dm = np.abs(c_t - c_e)
    D = d["dc2"]
    dD = float((2 * dm[1:] * em[1:] + em[1:] ** 2).sum()) + 2 * (P + 2) * U * D
    K = score.QUALITY_CD_SCALE
    cd_raw = K * math.sqrt(2 * D)
    cd = K * max(math.sqrt(2 * (D + dD)) - math.sqrt(2 * D), math.sqrt(2 * D) - math.sqrt(2 * max(D - dD, 0.0))) + 8 * U * cd_raw
    return {"cond_t": ct, "cond_e": ce, "r": ((N + 1) * U * d["r_t"][0], (N + 1) * U * d["r_e"][0]), "x": x, "llr": llr, "cd": cd,
            "llr_raw": raw, "cd_raw": cd_raw}


def _clamp_db(q):
    return min(max(score._db(q), score.QUALITY_SNR_MIN), score.QUALITY_SNR_MAX)


def fw_bar(tw, ew, X, Y, W, fw):
    """the bar of one kept frame's fw_f: tw, ew the windowed frames, X, Y its band sums [K] of the reference"""
    mags = [np.abs(np.fft.rfft(v, n=score.QUALITY_FFT)) for v in (tw, ew)]
    nz = (W != 0).sum(axis=1)
    dX, dY = (W @ (2 * C_F * U * float(np.abs(v).sum()) + 4 * U * m) + 2 * (nz + 1) * U * s for v, m, s in zip((tw, ew), mags, (X, Y)))
    g = X ** score.QUALITY_GAMMA
    dS = dG = 0.0
    for j in range(len(X)):
        s = score.QUALITY_SNR_MAX if X[j] == Y[j] else _clamp_db(score._div(X[j] * X[j], (X[j] - Y[j]) ** 2))
        dD, aD = dX[j] + dY[j], abs(X[j] - Y[j])
        hi = score.QUALITY_SNR_MAX if aD <= dD else _clamp_db(score._div((X[j] + dX[j]) ** 2, (aD - dD) ** 2))
        lo = _clamp_db(score._div(max(X[j] - dX[j], 0.0) ** 2, (aD + dD) ** 2))
        bs = max(hi - s, s - lo) + 16 * U * 45.0
        dg = max((X[j] + dX[j]) ** score.QUALITY_GAMMA - g[j], g[j] - max(X[j] - dX[j], 0.0) ** score.QUALITY_GAMMA) + 8 * U * g[j]
        dS += dg * (score.QUALITY_SNR_MAX - s) + g[j] * bs + dg * bs + 2 * (len(X) + 2) * U * g[j] * (score.QUALITY_SNR_MAX - s)
        dG += dg
    G = float(g.sum())
    dG += 2 * (len(X) + 1) * U * G
    assert G > 2 * dG, (G, dG)
    return (dS + (score.QUALITY_SNR_MAX - fw) * dG) / (G - dG) + 4 * U * 45.0


def reference_with_bars(e, t, bands=None):
    """-> (ref, bars): score.quality_reference with per_frame and details, and per frame the bars: "lpc" (lpc_bars or None
    where skipped), "fw" (float or None), and per figure of the record its bar"""
    ref = score.quality_reference(e, t, per_frame=True, bands=bands, details=True)
    n, w = ref["n"], score.quality_window()
    W = score.quality_band_matrix() if bands is None else np.asarray(bands, dtype=np.float64)
    ft = score.quality_frames(np.asarray(t[:n], np.float32).astype(np.float64), w)
    fe = score.quality_frames(np.asarray(e[:n], np.float32).astype(np.float64), w)
    X, Y = ref["band_sums"]
    per = ref["per_frame"]
    lpc = [lpc_bars(d) if d["ok"] else None for d in ref["lpc"]]
    fw = [fw_bar(ft[f], fe[f], X[f], Y[f], W, per[f, 2]) if per[f, 2] == per[f, 2] else None for f in range(ref["frames"])]
    return ref, record_bars({"lpc": lpc, "fw": fw}, per)


def record_bars(bars, per):
    """the frames' bars {"lpc", "fw"} and the per-frame values -> the same with the bars of the record's figures"""
    bars = {"lpc": bars["lpc"], "fw": bars["fw"]}
    lpc, fw = bars["lpc"], bars["fw"]
    for col, key, names in ((0, "llr", ("llr", "llr_95")), (1, "cd", ("cd_db", "cd_95_db"))):
        b = [x[key] for x in lpc if x is not None]
        v = [abs(per[f, col]) for f in range(len(per)) if lpc[f] is not None]
        q = (19 * len(b) + 10) // 20
        bars[names[0]] = sum(b) / len(b) + 2 * (len(b) + 2) * U * max(v) if b else 0.0
        bars[names[1]] = max(b) + 2 * (q + 4) * U * max(v) if b else 0.0
    b = [x for x in fw if x is not None]
    bars["fwsegsnr_db"] = sum(b) / len(b) + 2 * (len(b) + 2) * U * 45.0 if b else 0.0
    return bars


def prefix(ref, bars, n):
    """(ref, bars) of the first n samples of the pair: the frames are the pair's first ones, the record is formed anew"""
    M = score.quality_num_frames(n)
    per = ref["per_frame"][:M]
    out = dict(score.quality_summary(n, per), per_frame=per, lpc=ref["lpc"][:M], band_sums=tuple(x[:M] for x in ref["band_sums"]))
    return out, record_bars({"lpc": bars["lpc"][:M], "fw": bars["fw"][:M]}, per)


def conditions(ref, bars, exact=False):
    """The conditions on the reference alone (module docstring) -> the largest cond2(R) of a kept frame"""
    worst = 0.0
    per = ref["per_frame"]
    kept = [f for f in range(ref["frames"]) if bars["lpc"][f] is not None]
    for f in kept:
        b = bars["lpc"][f]
        worst = max(worst, b["cond_t"], b["cond_e"])
        assert b["x"] < 0.5, (f, b["x"])
        if not exact:
            assert 2 * b["llr"] < b["llr_raw"] < score.QUALITY_LLR_MAX - 2 * b["llr"] or b["llr_raw"] > score.QUALITY_LLR_MAX + 2 * b["llr"], (f, b)
            assert 2 * b["cd"] < b["cd_raw"] < score.QUALITY_CD_MAX - 2 * b["cd"] or b["cd_raw"] > score.QUALITY_CD_MAX + 2 * b["cd"], (f, b)
    assert worst <= COND_MAX, worst
    if kept and not exact:
        q = (19 * len(kept) + 10) // 20
        for col, key in ((0, "llr"), (1, "cd")):
            order = sorted(kept, key=lambda f: per[f, col])
            fq = order[q - 1]
            for f in kept:
                if f != fq and per[f, col] not in (0.0, score.QUALITY_LLR_MAX if col == 0 else score.QUALITY_CD_MAX):
                    assert abs(per[f, col] - per[fq, col]) > 2 * (bars["lpc"][f][key] + bars["lpc"][fq][key]), (key, f, fq)
    return worst


def quality_ratios(rec, per, ref, bars, lpc_rows=None):
    """The device's record (dict), per-frame values [M, 3] and (optionally) rows of nhans_quality_lpc against the reference
    -> {figure: worst |error| / bar}.  Counts and the kept frames must be equal."""
    for k in ("n", "frames", "frames_lpc", "frames_fw"):
        assert rec[k] == ref[k], (k, rec[k], ref[k])
    rp = ref["per_frame"]
    assert per.shape == rp.shape and np.array_equal(np.isnan(per), np.isnan(rp)), "the kept frames differ"
    assert not np.signbit(per[~np.isnan(per)][per[~np.isnan(per)] == 0.0]).any()
    out = {"llr_f": 0.0, "cd_f": 0.0, "fw_f": 0.0}
    for f in range(ref["frames"]):
        b = bars["lpc"][f]
        if b is not None:
            out["llr_f"] = max(out["llr_f"], abs(per[f, 0] - rp[f, 0]) / b["llr"])
            out["cd_f"] = max(out["cd_f"], abs(per[f, 1] - rp[f, 1]) / b["cd"])
            if lpc_rows is not None:
                d = ref["lpc"][f]
                got = max(np.abs(lpc_rows[f, :P + 1] - d["r_t"]).max() / b["r"][0], np.abs(lpc_rows[f, P + 1:2 * P + 2] - d["r_e"]).max() / b["r"][1])
                out["r"] = max(out.get("r", 0.0), float(got))
        if bars["fw"][f] is not None:
            out["fw_f"] = max(out["fw_f"], abs(per[f, 2] - rp[f, 2]) / bars["fw"][f])
    for k in score.QUALITY_FIGURES:
        if math.isnan(ref[k]):
            assert math.isnan(rec[k]), (k, rec[k])
        elif bars[k] == 0.0:
            assert rec[k] == ref[k], (k, rec[k], ref[k])
            out[k] = 0.0
        else:
            out[k] = abs(rec[k] - ref[k]) / bars[k]
    return out


# ---- the test signals ---------------------------------------------------------------------------------
def coloured(n, seed, poles=(1.2, -0.6)):
    """unit-variance AR(2) noise, x[i] = p0 x[i - 1] + p1 x[i - 2] + v[i], float64"""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -poles[0], -poles[1]], rng.standard_normal(n + 200))[200:]
    return x / (x.std() if n > 1 and x.std() > 0 else 1.0)


def clip(n, seed, noise=0.3, white=0.02):
    """(estimate, target) float32: the target AR(2) noise at level 0.1 with a white component `white` of its level (0.02:
    34 dB below), the estimate the target plus `noise` of another colour and its own white component"""
    rng = np.random.default_rng(10_000 + seed)
    t = 0.1 * (coloured(n, seed) + white * rng.standard_normal(n))
    e = t + 0.1 * noise * (coloured(n, seed + 5000, poles=(0.5, -0.3)) + white * rng.standard_normal(n))
    return e.astype(np.float32), t.astype(np.float32)


def periodic_clip(periods=14, seed=3):
    """both signals repeat with period 120 = the hop: every frame holds the same samples, every value is tied"""
    e, t = clip(H, 400 + seed, white=0.3)
    return np.tile(e, periods), np.tile(t, periods)


def zero_runs_clip(seed=5):
    """6,000 samples; zeros in the target at [0, 840) (leading), in the estimate at [2040, 2880) (inner), in both at
    [5160, 6000) (trailing): runs of 840 >= 720, at multiples of the hop"""
    e, t = clip(6000, 500 + seed)
    e, t = e.copy(), t.copy()
    t[:840] = 0.0
    e[2040:2880] = 0.0
    e[5160:] = 0.0
    t[5160:] = 0.0
    return e, t


def frames_to_samples(m):
    return N + H * (m - 1) if m > 0 else 0


# n = 0, 479, 480, 599, 600, 601; one sample either side of every edge of the LPC tile (7 frames: n = 1200, 2040; the
# frame after: 1320, 2160) and of the band tile (2 frames: 600, 840; the frame after: 720, 960); Mk = 1, 10, 11, 30
EDGES = sorted({frames_to_samples(m) + d for m in (LT, LT + 1, 2 * LT, 2 * LT + 1, BT, BT + 1, 2 * BT, 2 * BT + 1) for d in (-1, 0, 1)})
SIZES = sorted(set([0, 479, 480, 599, 600, 601] + EDGES + [frames_to_samples(m) for m in (1, 10, 11, 30)]))
LONG = 48000                                    # the 3 s clip
BASE = max(SIZES)                               # every size of SIZES is scored on the first n samples of ONE pair: clip(BASE, 11)


def base_clip():
    return clip(BASE, 11)


def custom_bands(K, seed=9):
    """a non-negative [K, 257] matrix: K = 1 all ones; else random rows, a third of the weights zero"""
    if K == 1:
        return np.ones((1, score.QUALITY_BINS))
    rng = np.random.default_rng(seed)
    W = rng.random((K, score.QUALITY_BINS))
    W[rng.random(W.shape) < 1 / 3] = 0.0
    return W


# ---- planted faults: the definition with one step wrong -> per-frame values [M, 3] --------------------------
def faulty_reference(e, t, fault):
    n = min(len(e), len(t))
    w = score.quality_window()
    x = [np.asarray(s[:n], np.float32).astype(np.float64) for s in (t, e)]
    if fault == "window_off_by_one":
        w = np.concatenate([w[1:], w[:1]])
    fr = [score.quality_frames(s, w) for s in x]
    per, rows = [], []
    for f in range(len(fr[0])):
        r = [score.quality_autocorr(fr[sg][f]) for sg in (0, 1)]
        if fault == "lag_dropped":                          # the lag list skips lag 8: chains 8 ... 16 work lags 9 ... 17
            lags = [k if k < 8 else k + 1 for k in range(P + 1)]
            r = [np.array([score._fsum((v[:N - k] * v[k:]).tolist()) for k in lags]) for v in (fr[0][f], fr[1][f])]
        a = [score.quality_levinson(v)[0] for v in r]
        num = score.quality_form(a[1], r[1] if fault == "wrong_R" else r[0])
        den = score.quality_form(a[0], r[0])
        c = []
        for aa in a:
            cc = np.zeros(P + 1)
            for m in range(1, P + 1):
                cc[m] = -aa[m] - score._fsum([((m - k) / m if fault == "k_over_m_swapped" else k / m) * cc[k] * aa[m - k] for k in range(1, m)])
            c.append(cc)
        dc2 = score._fsum(((c[0] - c[1])[1:] ** 2).tolist())
        ok = num > 0.0 and den > 0.0 and dc2 == dc2        # (a faulty lag list need not be positive definite: NaN then)
        per.append([min(max(math.log(num / den), 0.0), 2.0), min(max(score.QUALITY_CD_SCALE * math.sqrt(2 * dc2), 0.0), 10.0)] if ok else [NAN, NAN])
        rows.append(np.concatenate(r))
    return np.array(per), np.array(rows)


FAULTS = ("window_off_by_one", "lag_dropped", "wrong_R", "k_over_m_swapped")


# ---- what the library refuses, without a device -------------------------------------------------------
def check_refusals(lib, handle, buf=None, out=None):
    """buf / out: device pointers the calls must leave alone (the GPU test passes guarded buffers and looks at them
    afterwards); by default a pointer that is never followed."""
    buf = buf if buf is not None else ctypes.c_void_p(4096)
    out = out if out is not None else ctypes.c_void_p(8192)
    i64 = hip.i64_array
    dp = ctypes.POINTER(ctypes.c_double)

    def quality(est=buf, eoff=(0, 600, 1200), tgt=buf, toff=(0, 600, 1200), n=2, bands=None, K=0, rec=out, frames=None):
        W = None if bands is None else np.ascontiguousarray(bands, dtype=np.float64).ctypes.data_as(dp)
        rc = lib.nhans_quality(handle, est, i64(eoff) if eoff is not None else None, tgt, i64(toff) if toff is not None else None, n,
                               W, K, rec, frames, None)
        return rc, lib.nhans_last_error().decode()

    def lpc(est=buf, eoff=(0, 600, 1200), tgt=buf, toff=(0, 600, 1200), n=2, rows=out):
        rc = lib.nhans_quality_lpc(handle, est, i64(eoff) if eoff is not None else None, tgt, i64(toff) if toff is not None else None, n,
                                   rows, None)
        return rc, lib.nhans_last_error().decode()

    for call, name in ((quality, "nhans_quality:"), (lpc, "nhans_quality_lpc:")):
        rc, msg = call(n=-1)
        assert rc == -1 and name in msg and "negative clip count" in msg, msg
        for kw in ({"eoff": None}, {"toff": None}, {"rec": None} if call is quality else {"rows": None}):
            rc, msg = call(**kw)
            assert rc == -1 and "null" in msg, msg
        rc, msg = call(eoff=(0, 10, 5))
        assert rc == -1 and "clip 1" in msg and "estimate offsets descend" in msg, msg
        rc, msg = call(toff=(7, 3, 20))
        assert rc == -1 and "clip 0" in msg and "target offsets descend" in msg, msg
        rc, msg = call(est=None, eoff=(0, 0, 10))
        assert rc == -1 and "clip 1" in msg and "null buffer" in msg, msg
        rc, msg = call(tgt=None)
        assert rc == -1 and "clip 0" in msg and "null buffer" in msg, msg
        big = 2 ** 31
        rc, msg = call(eoff=(0, 10, 10 + big), toff=(0, 10, 10 + big))
        assert rc == -1 and "clip 1" in msg and "%d samples" % big in msg and "2^31 - 1" in msg, msg
    ones = np.ones((2, score.QUALITY_BINS))
    for K in (0, -1, 33):
        rc, msg = quality(bands=ones, K=K)
        assert rc == -1 and "%d bands" % K in msg and "1 ... 32" in msg, msg
    for bad in (-1e-300, float("nan"), float("inf")):
        W = ones.copy()
        W[1, 5] = bad
        rc, msg = quality(bands=W, K=2)
        assert rc == -1 and "[1, 5]" in msg and "negative or not finite" in msg, msg
    if handle is None:
        rc, msg = quality()
        assert rc < 0, msg                      # (what passes the checks meets the null context)
