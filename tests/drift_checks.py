"""What tests/test_drift_host.py and tests/test_gpu_drift.py share: the clips, the float64 bars, the device's own order
restated on the host, and the planted faults.

The bars.  U = 2^-53, B = 4096 samples a block.  The reference (nhans_amd.score.drift_reference) rounds every sum over
samples once (math.fsum of exact products); the device (drift.hip) adds the same exact products in a fixed order of its own.
  * c[d]: B exact terms added in any order take B - 1 roundings, each at most U times a partial sum that is at most
    A_d = sum |e t|, plus U A_d for the reference's one rounding:  bar_c[d] = B U A_d  (the bar of tests/align_checks.py).
  * a fine value v = the chain over 32 taps of fma(c[m + i], G[i], acc).  Both sides run the same chain on their own c: the
    difference of the inputs passes through with weights |G[i]|, and each side's chain rounds 32 times, each rounding at
    most U times a partial sum that is at most S = sum |c[m + i] G[i]|:   bar_v = sum |G[i]| bar_c[m + i] + 64 U S.
  * rho = v / sqrt(E_e E_t): E_e and E_t are sums of B exact squares each -- relative error B U each, half of it under the
    root --, 1.5 U for the product and the root, U for the quotient, either side:
        bar_rho = |rho| (bar_v / |v| + (2 B + 6) U).
  * u = j H + N / E_t: N's B terms are positive and each step of the device's chain rounds once (relative error B U), E_t
    likewise, the reference's two sums round once each, the quotient and the sum once on either side:
        bar_u = (N / E_t) (2 B + 6) U + 2 U |u|.
  * tau = (d* + k / 32) + delta, delta = ((v- - v+) / (2 den)) / 32, den = (v- - 2 v) + v+.  With ev the largest bar_v of the
    three, |d num| <= 2 ev + 2 U |num| and |d den| <= 4 ev + 4 U (|v-| + 2 |v| + |v+|); the quotient moves by at most
    (|d num| |den| + |num| |d den|) / (|den| (|den| - |d den|)) -- the test asserts |d den| < |den| / 2 on the reference --,
    the clamp moves nothing further, and the last operations round three times:
        bar_tau = that / 64 + 3 U |delta| + 2 U |tau|.
  * d*, k, the flags and z have no bar: they must be EQUAL, and `decided` asserts on the reference alone why they can be --
    the winning lag leads every other lag of the search by more than twice the largest bar_c, the winning fine value
    leads every other one by more than twice the largest bar_v -- or the block is silent.
  * the fit: nhans_drift_fit against score.drift_fit is held bit for bit.  The unit is compiled with contraction off
    (#pragma clang fp contract(off) at its head; the x86-64 baseline it is compiled for has no fused instruction either),
    so no bar applies.  The device's (a, b) against the reference's, both fitted from their own records: `fit_bar`
    propagates the records' bars through the fit numerically -- the line is re-fitted with every tau moved by +-bar_tau
    and every u by +-bar_u in the directions that move it most (the fit is linear in tau; u enters to first order) --
    and the bar is twice the largest movement seen.
  * the warp has no bar: it is held bit for bit to score.drift_warp_reference with the library's own table.
The worst measured ratios are in profiles/drift/README.md.

Planted faults (test_drift_host.py): each must leave its bar by orders of magnitude, so the bar is known to see them."""
import functools
import math

import numpy as np

from nhans_amd import hip, score

U = 2.0 ** -53
T, Q, B, H, F = hip.DRIFT_TAPS, hip.DRIFT_PHASES, hip.DRIFT_BLOCK, hip.DRIFT_HOP, hip.DRIFT_FINE
assert (T, Q, B, H, F, hip.DRIFT_TILE) == (16, 512, 4096, 2048, 32, 2048)
assert (T, Q, B, H, F) == (score.DRIFT_T, score.DRIFT_Q, score.DRIFT_BLOCK, score.DRIFT_HOP, score.DRIFT_FINE)
RATE = 16000


# ---- clips ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tones(seed, n=300, fmax=5000.0):
    rng = np.random.default_rng(7000 + seed)
    f = rng.uniform(80.0, fmax, n)
    return f, rng.uniform(0.2, 1.0, n) / np.sqrt(f / 80.0), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, 2)


def analytic_signal(x, seed):
    """s(x) at real positions x (samples at 16 kHz): 300 sinusoids below 5 kHz under a slow envelope, peak about 0.3"""
    f, amp, ph, eph = _tones(seed)
    x = np.asarray(x, np.float64)
    s = np.zeros(len(x))
    for k in range(0, len(f), 20):
        s += (amp[k:k + 20, None] * np.sin(2 * np.pi * f[k:k + 20, None] / RATE * x[None, :] + ph[k:k + 20, None])).sum(axis=0)
    env = 0.55 + 0.3 * np.sin(2 * np.pi * 0.9 / RATE * x + eph[0]) + 0.15 * np.sin(2 * np.pi * 3.1 / RATE * x + eph[1])
    return 0.02 * env * s


@functools.lru_cache(maxsize=None)
def analytic_clip(nt, a, b, snr_db, seed, extra=64):
    """-> (e [nt + extra], t [nt]) float32: t[u] = s(u) and e[v] = s((v - a) / (1 + b)) -- so that e at a + u + b u is t[u]
    exactly, before the float32 rounding -- plus white noise at snr_db below the estimate's power (None: none)"""
    t = analytic_signal(np.arange(nt), seed)
    e = analytic_signal((np.arange(nt + extra) - a) / (1.0 + b), seed)
    if snr_db is not None:
        rng = np.random.default_rng(8000 + seed)
        e = e + rng.standard_normal(len(e)) * math.sqrt(float(np.mean(e * e)) * 10.0 ** (-snr_db / 10.0))
    e, t = e.astype(np.float32), t.astype(np.float32)
    e.setflags(write=False)
    t.setflags(write=False)
    return e, t


# the clips of the issue: (samples, a, b, SNR dB, seed, max_lag, track_lag)
E2E_CLIPS = [
    (40000, 37.3, 50e-6, 60.0, 1, 400, 64),
    (40000, -20.75, -200e-6, 20.0, 2, 400, 64),
    (40000, 3.25, 500e-6, 10.0, 3, 400, 64),
    (160000, 11.6, 150e-6, 30.0, 4, 400, 32),       # 24 samples of drift over the clip
    (160000, 11.6, 150e-6, 30.0, 4, 400, 8),        # the same clip, tracked so narrowly that only the second pass reaches its ends
]


def e2e_clip(i):
    n, a, b, snr, seed, _, _ = E2E_CLIPS[i]
    return analytic_clip(n, a, b, snr, seed)


def noise_pair(ne, nt, seed, delay=None, level=0.1, noise=0.3):
    """white noise t and, with a delay, a copy `delay` samples late plus noise -- else independent noise -- float32"""
    rng = np.random.default_rng(9000 + seed)
    t = level * rng.standard_normal(nt)
    if delay is None:
        return (level * rng.standard_normal(ne)).astype(np.float32), t.astype(np.float32)
    s = np.concatenate([level * rng.standard_normal(4096), t, level * rng.standard_normal(abs(delay) + ne + 4096)])
    e = s[4096 - delay:4096 - delay + ne] + noise * level * rng.standard_normal(ne)
    return e.astype(np.float32), t.astype(np.float32)


# ---- the bars -------------------------------------------------------------------------------------
def corr_bars(e, t, j, z, R):
    """-> float64 [2 (R + T) + 1]: bar_c[d] = B U sum_i |e[j H + i + d] t[j H + i]|"""
    e, t = np.abs(np.asarray(e, np.float32).astype(np.float64)), np.abs(np.asarray(t, np.float32).astype(np.float64))
    tb = t[j * H:j * H + B]
    out = np.zeros(2 * (R + T) + 1)
    for n, d in enumerate(range(z - R - T, z + R + T + 1)):
        x0 = j * H + d
        lo, hi = max(0, -x0), min(B, len(e) - x0)
        if hi - lo > 1:
            out[n] = B * U * float(np.dot(e[x0 + lo:x0 + hi], tb[lo:hi])) * (1.0 + 2.0 ** -40)
    return out


def fine_bars(c, cbar, lm, G):
    """-> float64 [65]: bar_v of the fine values around index lm of the lag vector c with bars cbar"""
    k = np.arange(-F, F + 1)
    w = k // F
    rows = np.abs(G[(Q // F) * (k - F * w)])
    out = np.zeros(len(k))
    for n in range(len(k)):
        l = lm + w[n] + np.arange(2 * T) - (T - 1)
        ok = (l >= 0) & (l < len(c))
        out[n] = float(np.dot(rows[n][ok], cbar[l[ok]]) + 64 * U * np.dot(rows[n][ok], np.abs(c[l[ok]])))
    return out * (1.0 + 2.0 ** -40)


def segment_bars(ref, cbar, R, G):
    """The bars of one segment's record from its reference record (with "corr") -> dict u, tau, rho, v, plus "decided": the
    least lead of the two winners over their rivals in units of twice the largest bar (above 1: equality can be asked)."""
    c = ref["corr"]
    lm = ref["d_int"] - ref["z"] + R + T
    vb = fine_bars(c, cbar, lm, G)
    fine, k = ref["fine"], ref["k"]
    silent = bool(ref["flags"] & score.DRIFT_SILENT)
    lead = math.inf
    if not silent:
        search = c[T:T + 2 * R + 1]
        rivals = np.delete(search, lm - T)
        if len(rivals) and cbar.max() > 0:
            lead = min(lead, float(c[lm] - rivals.max()) / (2.0 * float(cbar.max())))
        if vb.max() > 0:
            lead = min(lead, float(fine[k + F] - np.delete(fine, k + F).max()) / (2.0 * float(vb.max())))
    v = ref["v_peak"]
    bar_tau = 2 * U * abs(ref["tau"])
    if -F < k < F and not silent:
        vm, vp = float(fine[k + F - 1]), float(fine[k + F + 1])
        ev = float(vb[k + F - 1:k + F + 2].max())
        num, den = vm - vp, (vm - 2.0 * v) + vp
        if den < 0.0:
            dnum = 2 * ev + 2 * U * abs(num)
            dden = 4 * ev + 4 * U * (abs(vm) + 2 * abs(v) + abs(vp))
            assert dden < abs(den) / 2, "the parabola's curvature %.3e is not decided (bar %.3e)" % (den, dden)
            bar_tau += (dnum * abs(den) + abs(num) * dden) / (abs(den) * (abs(den) - dden)) / 64.0 + 3 * U * abs(ref["delta"])
    with np.errstate(all="ignore"):
        bar_rho = abs(ref["rho"]) * (float(vb[k + F]) / abs(v) + (2 * B + 6) * U) if math.isfinite(ref["rho"]) and v != 0.0 else 0.0
    bar_u = (ref["u"] - ref["u0"]) * (2 * B + 6) * U + 2 * U * abs(ref["u"]) if math.isfinite(ref["u"]) else 0.0
    return {"u": bar_u, "tau": bar_tau, "rho": bar_rho, "v": float(vb[k + F]), "decided": lead}


def ratio(got, ref, bar):
    """|got - ref| / bar; values that are not finite must be THE SAME non-finite value (ratio 0), else inf."""
    got, ref = float(got), float(ref)
    if not (math.isfinite(got) and math.isfinite(ref)):
        same = (math.isnan(got) and math.isnan(ref)) or got == ref
        return 0.0 if same else math.inf
    if got == ref:
        return 0.0
    return abs(got - ref) / bar if bar > 0 else math.inf


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def same_f32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def reference_segments(e, t, ca, cb, R, table=None):
    """score.drift_reference with the lag vectors, each record with its u0 = j H and its bars -> list of (record, bars, bar_c)"""
    G = (table or score.drift_table())[0]
    out = []
    for j, ref in enumerate(score.drift_reference(e, t, ca, cb, R, corr=True, table=table)):
        ref["u0"] = j * H
        cbar = corr_bars(e, t, j, ref["z"], R)
        out.append((ref, segment_bars(ref, cbar, R, G), cbar))
    return out


def segment_ratios(got, gcorr, ref, bars, cbar):
    """got: dict by score.DRIFT_FIELDS, gcorr: its lag vector -> {"corr", "u", "tau", "rho", "v"}: the worst ratios; what has no
    bar must be equal."""
    for k in ("d_int", "flags", "z"):
        assert int(got[k]) == int(ref[k]), (k, got[k], ref[k])
    diff = np.abs(np.asarray(gcorr, np.float64) - ref["corr"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0.0, 0.0, np.where(cbar > 0, diff / cbar, np.inf))
    out = {"corr": float(r.max()), "v": ratio(got["v_peak"], ref["v_peak"], bars["v"])}
    out.update({k: ratio(got[k], ref[k], bars[k]) for k in ("u", "tau", "rho")})
    er = ratio(got["E_t"], ref["E_t"], B * U * ref["E_t"])
    out["E_t"] = er
    return out


def fit_bar(refs, rho_min=score.DRIFT_RHO_MIN, trim=score.DRIFT_TRIM):
    """refs: [(record, bars, ...)] of one clip -> (bar_a, bar_b): twice the largest movement of the fitted line when every tau
    and u moves by its bar in the directions that move the line most (see the head of the file)"""
    base = score.drift_fit([r[0] for r in refs], rho_min, trim)
    if not base["fit_ok"]:
        return 0.0, 0.0
    us = np.array([r[0]["u"] for r in refs])
    mid = float(np.nanmean(us))
    worst = [0.0, 0.0]
    for pattern in (lambda u: 1.0, lambda u: 1.0 if u >= mid else -1.0):
        for su in (0.0, 1.0, -1.0):
            moved = []
            for r in refs:
                sgn = pattern(r[0]["u"]) if math.isfinite(r[0]["u"]) else 0.0
                moved.append(dict(r[0], tau=r[0]["tau"] + sgn * r[1]["tau"], u=r[0]["u"] + su * sgn * r[1]["u"]))
            f = score.drift_fit(moved, rho_min, trim)
            worst = [max(worst[0], abs(f["a"] - base["a"])), max(worst[1], abs(f["b"] - base["b"]))]
    return 2.0 * worst[0] + 4 * U * abs(base["a"]), 2.0 * worst[1] + 4 * U * abs(base["b"])


def coarse_delay(e, t, max_lag):
    """the whole-sample delay within max_lag by an FFT cross-correlation in float64 (the clips here decide it by a wide
    margin; the GPU tests hold Context.align to score.align_reference elsewhere)"""
    n = 1 << int(math.ceil(math.log2(len(e) + len(t))))
    c = np.fft.irfft(np.fft.rfft(np.asarray(e, np.float64), n) * np.conj(np.fft.rfft(np.asarray(t, np.float64), n)), n)
    lags = np.arange(-max_lag, max_lag + 1)
    return int(lags[int(np.argmax(c[lags % n]))])


@functools.lru_cache(maxsize=None)
def reference_line(i):
    """Context.align_drift of E2E clip i restated on the reference -> (fit dict with d0, the segments of the last pass as
    reference_segments gives them, the radius of that pass, the centre line of that pass)"""
    e, t = e2e_clip(i)
    max_lag, track_lag = E2E_CLIPS[i][5:7]
    d0 = coarse_delay(e, t, max_lag)
    centre, R = (float(d0), 0.0), track_lag
    refs = reference_segments(e, t, centre[0], centre[1], R)
    fit = score.drift_fit([r[0] for r in refs])
    if fit["fit_ok"]:
        centre, R = (fit["a"], fit["b"]), 8
        refs = reference_segments(e, t, centre[0], centre[1], R)
        fit = score.drift_fit([r[0] for r in refs])
    return dict(fit, d0=d0), refs, R, centre


def si_sdr_db(e, t):
    e, t = np.asarray(e, np.float64), np.asarray(t, np.float64)
    alpha = float(np.dot(e, t) / np.dot(t, t))
    return 10.0 * math.log10(float(np.dot(alpha * t, alpha * t)) / float(np.dot(e - alpha * t, e - alpha * t)))


# ---- the device's own order on the host ----------------------------------------------------------------
def _tree(v):
    """thread l's value v[l], l < 256, summed by the tree 128, ..., 1"""
    v = np.array(v, np.float64)
    off = 128
    while off:
        v[:off] = v[:off] + v[off:2 * off]
        off >>= 1
    return float(v[0])


def _strided(x, fused_index=False):
    """thread l adds x[l], x[l + 256], ... in one chain from +0.0 (fused_index: acc = fma(i, x[i], acc)), then the tree"""
    rows = np.asarray(x, np.float64).reshape(-1, 256)
    acc = np.zeros(256)
    for r in range(rows.shape[0]):
        acc = score._fma(np.arange(256.0) + 256.0 * r, rows[r], acc) if fused_index else acc + rows[r]
    return _tree(acc)


def device_order_segment(e, t, j, z, R, table):
    """Segment j's record and lag vector in the order drift.hip states, operation by operation: what the device must give
    bit for bit -> (dict by score.DRIFT_FIELDS plus k, float64 [2 (R + T) + 1])"""
    e, t = np.asarray(e, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    tb = t[j * H:j * H + B]
    nl = 2 * (R + T) + 1
    x0 = j * H + z - R - T
    win = np.zeros(B + nl - 1)
    lo, hi = max(0, -x0), min(len(win), len(e) - x0)
    if hi > lo:
        win[lo:hi] = e[x0 + lo:x0 + hi]
    c = np.zeros(nl)
    TS = hip.DRIFT_TILE
    for l in range(nl):
        prod = win[l:l + B] * tb                      # exact: a fused multiply-add of it is a plain addition
        c[l] = float(np.cumsum(prod[:TS])[-1]) + float(np.cumsum(prod[TS:])[-1])
    sq = tb * tb
    Et, N = _strided(sq), _strided(sq, fused_index=True)

    def Ee_of(d):
        w = win[d - z + R + T:d - z + R + T + B]
        return _strided(w * w)

    rec = score.drift_peak(c, R, z, Et, Ee_of, j * H, N, table[0])
    return rec, c


# ---- planted faults: the definition put together wrongly ------------------------------------------------
def fault_block_centre(refs):
    """the abscissa is the block's centre, not its energy centroid"""
    return [dict(r[0], u=r[0]["u0"] + 0.5 * (B - 1)) for r in refs]


def fault_hop_off_by_one(e, t, ca, cb, R):
    """the blocks are taken at hop H + 1 (the records still claim hop H)"""
    e64, t64 = np.asarray(e, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    G = score.drift_table()[0]
    out = []
    for j, z in enumerate(score.drift_centres(ca, cb, score.drift_segments(len(t)))):
        s = j * (H + 1)
        if s + B > len(t):
            break
        tb = t64[s:s + B]
        c = np.array([score.drift_lag_sum(e64, tb, s + d) for d in range(z - R - T, z + R + T + 1)])
        Et, N = score._drift_moment(tb)
        out.append(score.drift_peak(c, R, z, Et, lambda d: 1.0, j * H, N, G))
    return out


def fault_warp(e, nt, a, b, table, tap_shift=0, drop_lambda=False):
    """score.drift_warp_reference with the tap index off by tap_shift, or with lambda dropped (the row G[q] alone)"""
    G, D = table
    e = np.asarray(e, np.float32).astype(np.float64)
    u_lo, u_hi = score.drift_range(len(e), nt, a, b)
    p = score.drift_pos(a, b, np.arange(u_lo, u_hi, dtype=np.float64))
    fl = np.floor(p)
    m = fl.astype(np.int64)
    f = (p - fl) * Q
    q = np.minimum(f.astype(np.int64), Q - 1)
    lam = np.zeros(len(p)) if drop_lambda else f - q
    acc = np.zeros(len(p))
    for j in range(2 * T):
        x = m + j - (T - 1) + tap_shift
        ok = (x >= 0) & (x < len(e))
        acc = score._fma(np.where(ok, e[np.clip(x, 0, len(e) - 1)], 0.0), score._fma(lam, D[q, j], G[q, j]), acc)
    return acc.astype(np.float32)


def fault_pos(a, b, u):
    """p computed as a + (1 + b) u: the sum 1 + b rounded, the product rounded, the sum rounded -- one rounding fewer than
    it takes to be right, and not the device's expression"""
    return a + (1.0 + b) * np.asarray(u, np.float64)


def brute_range(ne, nt, a, b, pos=score.drift_pos):
    u = np.arange(nt, dtype=np.float64)
    p = pos(a, b, u)
    idx = np.nonzero((p >= 0) & (p <= ne - 1))[0]
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


# ---- the refusals, each by its message (no device is touched: handle may be None) ----------------------------
def check_refusals(lib, handle, buf=None, out=None):
    """buf / out: device pointers the calls must leave alone (the GPU test passes guarded buffers and looks at them
    afterwards); by default a pointer that is never followed."""
    import ctypes
    buf = buf if buf is not None else ctypes.c_void_p(4096)
    out = out if out is not None else ctypes.c_void_p(8192)
    i64, dbl = hip.i64_array, hip.dbl_array
    opt = lambda f, v: f(v) if v is not None else None

    def track(est=buf, eoff=(0, 5000, 10000), tgt=buf, toff=(0, 5000, 10000), n=2, ca=(0.0, 1.0), cb=(0.0, 0.0), R=8, rec=out, corr=None):
        rc = lib.nhans_drift_track(handle, est, opt(i64, eoff), tgt, opt(i64, toff), n, opt(dbl, ca), opt(dbl, cb), R, rec, corr, None)
        return rc, lib.nhans_last_error().decode()

    def warp(est=buf, eoff=(0, 100, 200), toff=(0, 100, 200), n=2, a=(0.0, 1.0), b=(0.0, 0.0), o=out, ooff=(0, 100, 200)):
        rc = lib.nhans_drift_warp(handle, est, opt(i64, eoff), opt(i64, toff), n, opt(dbl, a), opt(dbl, b), o, opt(i64, ooff), None)
        return rc, lib.nhans_last_error().decode()

    rc, msg = track(n=-1)
    assert rc == -1 and "negative clip count" in msg, msg
    for R in (0, -1, 1025, 1 << 20):
        rc, msg = track(R=R)
        assert rc == -1 and "radius %d" % R in msg and "1 ... 1024" in msg, msg
    for kw in ({"rec": None}, {"eoff": None}, {"toff": None}, {"ca": None}, {"cb": None}):
        rc, msg = track(**kw)
        assert rc == -1 and "null" in msg, msg
    rc, msg = track(eoff=(0, 10, 5))
    assert rc == -1 and "clip 1" in msg and "estimate offsets descend" in msg, msg
    rc, msg = track(toff=(7, 3, 20))
    assert rc == -1 and "clip 0" in msg and "target offsets descend" in msg, msg
    rc, msg = track(est=None, eoff=(0, 0, 10))
    assert rc == -1 and "clip 1" in msg and "null buffer" in msg, msg
    rc, msg = track(tgt=None)
    assert rc == -1 and "clip 0" in msg and "null buffer" in msg, msg
    rc, msg = track(toff=(0, 10, 10 + 2 ** 31))
    assert rc == -1 and "clip 1" in msg and "%d samples" % 2 ** 31 in msg and "2^31 - 1" in msg, msg
    rc, msg = track(cb=(0.0, 2.0 ** -10 * (1 + 2.0 ** -52)))
    assert rc == -1 and "clip 1" in msg and "drift" in msg and "2^-10" in msg, msg
    for bad in (math.nan, math.inf):
        rc, msg = track(ca=(bad, 0.0))
        assert rc == -1 and "clip 0" in msg and "not finite" in msg, msg
        rc, msg = track(cb=(0.0, -bad))
        assert rc == -1 and "clip 1" in msg and "not finite" in msg, msg
    rc, msg = track(ca=(0.0, 2.0 ** 31 - 10))
    assert rc == -1 and "clip 1" in msg and "int32 range" in msg and "segment 0" in msg, msg
    rc, msg = track(ca=(-2.0 ** 31 - 1, 0.0))
    assert rc == -1 and "clip 0" in msg and "int32 range" in msg, msg

    rc, msg = warp(n=-1)
    assert rc == -1 and "negative clip count" in msg, msg
    for kw in ({"eoff": None}, {"toff": None}, {"a": None}, {"b": None}, {"o": None}, {"ooff": None}):
        rc, msg = warp(**kw)
        assert rc == -1 and "null" in msg, msg
    rc, msg = warp(est=None)
    assert rc == -1 and "clip 0" in msg and "null buffer" in msg, msg
    rc, msg = warp(eoff=(0, 10, 5))
    assert rc == -1 and "clip 1" in msg and "estimate offsets descend" in msg, msg
    rc, msg = warp(toff=(0, 10, 9))
    assert rc == -1 and "clip 1" in msg and "target offsets descend" in msg, msg
    rc, msg = warp(ooff=(5, 2, 300))
    assert rc == -1 and "clip 0" in msg and "output offsets descend" in msg, msg
    rc, msg = warp(b=(0.0, -0.001))
    assert rc == -1 and "clip 1" in msg and "drift" in msg and "2^-10" in msg, msg
    for bad in (math.nan, -math.inf):
        rc, msg = warp(a=(0.0, bad))
        assert rc == -1 and "clip 1" in msg and "not finite" in msg, msg
        rc, msg = warp(b=(bad, 0.0))
        assert rc == -1 and "clip 0" in msg and "not finite" in msg, msg
    rc, msg = warp(a=(3e9, 0.0))
    assert rc == -1 and "clip 0" in msg and "int32 range" in msg, msg
    rc, msg = warp(ooff=(0, 100, 198))                     # clip 1: a = 1 leaves 99 samples
    assert rc == -1 and "clip 1" in msg and "output room" in msg and "98 samples, 99 needed" in msg, msg
    rc, msg = warp(toff=(0, 100, 100 + 2 ** 31))
    assert rc == -1 and "clip 1" in msg and "2^31 - 1" in msg, msg

    lo, hi = ctypes.c_int64(7), ctypes.c_int64(7)
    assert lib.nhans_drift_range(10, 10, 0.0, 0.002, ctypes.byref(lo), ctypes.byref(hi)) == -1 and "2^-10" in lib.nhans_last_error().decode()
    assert lib.nhans_drift_range(10, 10, math.nan, 0.0, ctypes.byref(lo), ctypes.byref(hi)) == -1 and "not finite" in lib.nhans_last_error().decode()
    assert lib.nhans_drift_range(-1, 10, 0.0, 0.0, ctypes.byref(lo), ctypes.byref(hi)) == -1 and "samples" in lib.nhans_last_error().decode()
    assert lib.nhans_drift_range(10, 10, 0.0, 0.0, None, ctypes.byref(hi)) == -1 and "null" in lib.nhans_last_error().decode()
    assert (lo.value, hi.value) == (7, 7)
    o6 = (ctypes.c_double * 6)(*([7.0] * 6))
    assert lib.nhans_drift_fit(None, -1, 0.3, 1.0, o6) == -1 and "negative segment count" in lib.nhans_last_error().decode()
    assert lib.nhans_drift_fit(None, 2, 0.3, 1.0, o6) == -1 and "null" in lib.nhans_last_error().decode()
    assert lib.nhans_drift_fit(dbl([0.0] * 8), 1, 0.3, 1.0, None) == -1 and "null" in lib.nhans_last_error().decode()
    assert lib.nhans_drift_fit(dbl([0.0] * 8), 1, 0.3, -1.0, o6) == -1 and "trim" in lib.nhans_last_error().decode()
    assert list(o6) == [7.0] * 6
    assert lib.nhans_drift_segments(B - 1) == 0 and lib.nhans_drift_segments(B) == 1 and lib.nhans_drift_segments(B + H - 1) == 1
    assert lib.nhans_drift_segments(B + H) == 2 and lib.nhans_drift_segments(0) == 0
