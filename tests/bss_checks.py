"""What tests/test_bss_host.py and tests/test_gpu_bss.py share: the clips, the float64 bar and the planted faults.

The bar.  The reference (nhans_amd.score.bss_reference) rounds every correlation once (math.fsum), solves with LAPACK's
Cholesky and projects with np.convolve; the device (bsseval.hip) adds in fixed orders of its own, factors with its own
blocked Cholesky and projects with one fused multiply-add chain per sample.  U = 2^-53, M = J L, S the (n + L - 1) x M
matrix of the shifted sources, G = S^T S, D = S^T e, lmin the least eigenvalue of G: cond_2(G) = |G|_2 / lmin.

  * Correlations.  A sum of exact products a[t] b[t + d] added in any order of at most K additions per term is off by
    K U sum |a b| <= K U sqrt(|a|^2 |b|^2) (Cauchy-Schwarz).  On the device K = K_CORR = tile + tiles + 2 (a chain inside a
    tile, then the tiles), in the reference 1.  Element (i, j) of G is therefore off by (K_CORR + 1) U sqrt(G_ii G_jj) -- a
    rank-one bound whose 2-norm is its trace -- and D by (K_CORR + 1) U sqrt(E_e trace G) in the 2-norm.
  * Cholesky.  The computed solution of either side solves (G + dG) C = D exactly with |dG| <= (3 M + 1) U |R| |R^T|
    elementwise (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.4: the backward error of order
    M U the issue names); the 2-norm of |R| |R^T| is taken from the reference's own factor.  Two sides: twice.
    Together  B_G = (K_CORR + 1) U trace G + 2 (3 M + 1) U | |R| |R^T| |_2   and   B_D = (K_CORR + 1) U sqrt(E_e trace G).
  * Coefficients and projections.  To first order dC = G^-1 r with r = dD - dG C, |r| <= B_D + B_G |C|.  So
        |dC| <= |r| / lmin = cond_2(G) |r| / |G|     and     |dP|^2 = |S dC|^2 = r^T G^-1 r <= |r|^2 / lmin,
    the second being the issue's |dP|^2 <= |G| |dC|^2 with the factor sqrt(cond) it gives away taken back (S dC sees
    G^-1 once, not twice).  The chain of M products behind a sample of P is off by (M + 2) U |C| |window|, and the
    squared windows sum to trace G: |dP_fir| <= (M + 2) U |C| sqrt(trace G) on either side.  s_target likewise from the
    leading block G_00, D[:L], C0 and L.
  * Energies.  E = |x|^2 of a vector off by d in the 2-norm is off by 2 |x| d + d^2, plus (K_SUM + 4) U E for the
    sum itself, K_SUM = 4 + 8 + tiles + 2 on the device.  d is dP for e_artif, ds for s_target and e - s_target,
    dP + ds for e_interf, dP + 2 ds for s_target + e_interf, each plus 2 U |x| for the subtraction; E_e has no d.
    The bar of an energy is that over E_e.
  * Figures.  10 log10(A / B) is off by (10 / ln 10) (dA / A + dB / B + 8 U).

C_BAR = 2 is the stated constant on all of it, for the second-order terms dropped above.  It is not tuned: the worst
measured ratio to the bar is in profiles/bsseval/README.md, and a ratio above one half would be a defect to find.

Two conditions keep the bar honest; `bss_bar` asserts the first on the reference alone for every clip held to it, and
`bss_ratios` applies the second:
  1. no pivot of the reference's factor is within a factor MARGIN = 1e6 of the singular threshold J L 2^-52 G_kk, so the
     decision cannot flip on a rounding;
  2. the cap: a dB figure is compared only if its bar is below CAP = 1e-3 dB; otherwise only its energies are compared.
     The one case allowed to drop a figure is SAR where the estimate lies in the span of the sources (its artifact term
     is rounding noise): the caller names the figures it allows to drop, and any other dropped figure fails.
A figure the definition makes infinite (SIR with one source) must be the same infinity on both sides.

Which shapes can be held to the bar.  With two sources G is 2 L x 2 L and has rank at most n + L - 1: below n = L + 1 it
is singular by construction and just above it is singular to rounding, so condition 1 fails on the reference and the
flag is a coin toss on either side.  Those shapes (EDGE_SHAPES) are run for what can be asserted of them -- the counts,
the flag in {0, 1}, NaN figures where it is 1, the same bits alone and in a batch -- and every other shape is held to
the bar.

Planted faults (test_bss_host.py): each must leave the bar by orders of magnitude, so the bar is known to see them."""
import math

import numpy as np

from nhans_amd import hip, score

U = 2.0 ** -53
C_BAR = 2.0
MARGIN = 1e6
CAP = 1e-3
DB = 10.0 / math.log(10.0)
CORR_TILE, PROJ_TILE = hip.BSS_CORR_TILE, 1024
# (L, J, n, AR coefficient): every L of {1, 2, 16, 100, 512} with either J; n of {1, L - 1, L, L + 1} with one source, where
# they are well posed; one correlation tile - 1, + 1 and exact; one projection tile - 1 and + 1 (n + L - 1 = 1023, 1025);
# 4000 and 16000
SHAPES = [(1, 1, 1, 0.5), (1, 1, 2, 0.5), (1, 1, 1023, 0.9), (1, 1, 1025, 0.9), (1, 2, 4000, 0.5), (2, 1, 1, 0.5), (2, 1, 2, 0.5), (2, 1, 3, 0.5),
          (2, 2, 1024, 0.9), (2, 2, 2049, 0.99), (16, 1, 1, 0.5), (16, 1, 15, 0.5), (16, 1, 16, 0.5), (16, 1, 17, 0.9), (16, 2, 2047, 0.5),
          (16, 2, 4000, 0.9), (16, 1, 16000, 0.99), (100, 1, 99, 0.5), (100, 1, 101, 0.5), (100, 2, 2048, 0.9), (100, 2, 4000, 0.5),
          (512, 1, 511, 0.5), (512, 1, 513, 0.5), (512, 1, 4000, 0.99), (512, 2, 2049, 0.9), (512, 2, 16000, 0.99)]
# two sources and n + L - 1 < 2 L, or barely more: rank-deficient by construction (see above)
EDGE_SHAPES = [(1, 2, 1, 0.5), (2, 2, 1, 0.5), (2, 2, 2, 0.5), (2, 2, 3, 0.5), (16, 2, 15, 0.5), (16, 2, 16, 0.5), (16, 2, 17, 0.5),
               (100, 2, 101, 0.5), (512, 2, 511, 0.5), (512, 2, 513, 0.5)]



def may_drop(shape):
    """The figures a shape may drop at the cap: a clip of one sample is a multiple of s_0's one sample, so the estimate
    lies in the span of the sources and the distortion and artifact terms are rounding noise."""
    return ("sdr_db", "sar_db") if shape[2] == 1 else ()


# ---- clips ----------------------------------------------------------------------------------------
def ar1(n, a, rng):
    """AR(1) coloured noise of unit innovation, scaled to speech-like level, float32"""
    w = rng.standard_normal(n)
    x = np.empty(n)
    p = 0.0
    for i in range(n):
        p = a * p + w[i]
        x[i] = p
    return (0.1 * math.sqrt(1.0 - a * a) * x).astype(np.float32)


def shift(x, k):
    return np.concatenate([np.zeros(k, x.dtype), x[:len(x) - k]]) if k else x


def clip(n, a, seed, J=2):
    """-> (estimate, [s_0] or [s_0, s_1]) float32 [n]: e = 0.8 s_0 + 0.1 shift(s_0, 3) + 0.2 s_1 + 0.05 white (the s_1 term is
    in the estimate with one source too: it is then noise)"""
    rng = np.random.default_rng(3000 + seed)
    s0, s1 = ar1(n, a, rng), ar1(n, a, rng)
    w = (0.1 * rng.standard_normal(n)).astype(np.float32)
    e = (0.8 * s0 + 0.1 * shift(s0, min(3, n)) + 0.2 * s1 + 0.05 * w).astype(np.float32)
    return e, [s0, s1][:J]


def shape_clip(shape, seed=0):
    L, J, n, a = shape
    return clip(n, a, 17 * seed + L + 7 * J + n, J)


# ---- the bar --------------------------------------------------------------------------------------
def _tiles(n, tile):
    return -(-n // tile)


def bss_bar(e, sources, L, ref=None):
    """-> (reference record with filters, {energy: bar relative to E_e, figure: bar in dB, "normal": bar on |G C - D|_2,
    "normal0": on |G_00 C0 - D[:L]|_2}); asserts condition 1.  A singular reference has no bar: None."""
    ref = ref or score.bss_reference(e, sources, L, filters=True)
    if ref["singular"]:
        return ref, None
    assert ref["pivot_margin"] >= MARGIN, "pivot margin %.3e" % ref["pivot_margin"]
    n, J = ref["n"], ref["J"]
    M = J * L
    G, D, C, C0 = ref["G"], ref["D"], ref["C"].reshape(-1), ref["C0"]
    k_corr = min(n, CORR_TILE) + _tiles(n, CORR_TILE) + 2 + 1
    k_sum = PROJ_TILE // 256 + 8 + _tiles(n + L - 1, PROJ_TILE) + 2 + 4
    E_e = ref["E_e"]

    def system(G, D, C, m):
        R = np.linalg.cholesky(G)
        tr = float(np.trace(G))
        b_g = k_corr * U * tr + 2.0 * (3 * m + 1) * U * float(np.linalg.norm(np.abs(R) @ np.abs(R.T), 2))
        b_d = k_corr * U * math.sqrt(E_e * tr)
        r = b_d + b_g * float(np.linalg.norm(C))
        lmin = float(np.linalg.eigvalsh(G)[0])
        assert lmin > 0
        return r, r / math.sqrt(lmin) + 2.0 * (m + 2) * U * float(np.linalg.norm(C)) * math.sqrt(tr)

    rP, dP = system(G, D, C, M)
    rs, ds = system(G[:L, :L], D[:L], C0, L)
    d = {"E_e": 0.0, "E_tgt": ds, "E_int": dP + ds, "E_art": dP, "E_dist": ds, "E_ti": dP + 2.0 * ds}
    abs_bar = {}
    for k in score.BSS_ENERGIES:
        x = math.sqrt(ref[k])
        dk = d[k] + 2.0 * U * x
        abs_bar[k] = C_BAR * (2.0 * x * dk + dk * dk + k_sum * U * ref[k])
    bar = {k: abs_bar[k] / E_e for k in score.BSS_ENERGIES}
    for fig, (a, b) in (("sdr_db", ("E_tgt", "E_dist")), ("sir_db", ("E_tgt", "E_int")), ("sar_db", ("E_ti", "E_art"))):
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = [float(np.float64(abs_bar[k]) / np.float64(ref[k])) for k in (a, b)]
        bar[fig] = DB * (rel[0] + rel[1] + C_BAR * 8.0 * U) if all(math.isfinite(v) for v in rel) else math.inf
    bar["normal"], bar["normal0"] = C_BAR * rP, C_BAR * rs
    return ref, bar


def ratio(got, ref, bar):
    """|got - ref| / bar; values that are not finite must be THE SAME non-finite value (ratio 0), else inf."""
    got, ref = float(got), float(ref)
    if not (math.isfinite(got) and math.isfinite(ref)):
        same = (math.isnan(got) and math.isnan(ref)) or got == ref
        return 0.0 if same else math.inf
    if got == ref:
        return 0.0
    return abs(got - ref) / bar if bar > 0 else math.inf


def bss_ratios(got, e, sources, L, may_drop=(), ref=None):
    """got: dict by score.BSS_FIELDS -> {energy or figure: ratio to the bar}; the counts and the flag must be equal.  A
    figure whose bar is not below CAP is dropped -- its energies are still compared -- and must be named in may_drop."""
    ref, bar = bss_bar(e, sources, L, ref)
    for k in ("n", "J", "L", "singular"):
        assert int(got[k]) == ref[k], (k, got[k], ref[k])
    if bar is None:
        return {k: ratio(got[k], ref[k], 0.0) for k in score.BSS_ENERGIES + score.BSS_FIGURES}
    out = {k: ratio(got[k] / ref["E_e"], ref[k] / ref["E_e"], bar[k]) for k in score.BSS_ENERGIES}
    for k in score.BSS_FIGURES:
        if k in may_drop and not (math.isfinite(ref[k]) and bar[k] < CAP):
            continue
        if not math.isfinite(ref[k]):
            out[k] = ratio(got[k], ref[k], 0.0)
        elif bar[k] < CAP:
            out[k] = ratio(got[k], ref[k], bar[k])
        else:
            assert k in may_drop, "%s dropped: its bar is %.3e dB" % (k, bar[k])
    return out


# ---- planted faults: the reference's steps put together wrongly ------------------------------------
def _faulty(e, sources, L, lag_off=False, unpadded=False, c0_from_c=False, cut=False):
    n = min([len(e)] + [len(s) for s in sources])
    e = np.asarray(e[:n], np.float32).astype(np.float64)
    src = [np.asarray(s[:n], np.float32).astype(np.float64) for s in sources]
    r, q = score.bss_correlations(e, src, L)
    if lag_off:                 # r_01[d] read one lag off
        r[0][1] = np.concatenate([r[0][1][1:], [0.0]])
        r[1][0] = r[0][1][::-1].copy()
    if unpadded:                # D from the windows of the estimate that fit into its n samples: t <= n - L
        q = [np.array([score._fsum((e[b:n - L + 1 + b] * s[:n - L + 1]).tolist()) for b in range(L)]) for s in src]
    G, D = score.bss_gram(r, q, L)
    C, C0, _ = score.bss_solve(G, D, L)
    if c0_from_c:
        C0 = C[:L]
    P, st = score.bss_project(C, C0, src, L)
    if cut:                     # the projections end with the signals
        P, st = np.concatenate([P[:n], np.zeros(L - 1)]), np.concatenate([st[:n], np.zeros(L - 1)])
    return dict({"n": n, "J": len(src), "L": L, "singular": 0}, **score.bss_figures(e, P, st, L))


def fault_lag_off_in_r01(e, sources, L):
    return _faulty(e, sources, L, lag_off=True)


def fault_unpadded_estimate(e, sources, L):
    return _faulty(e, sources, L, unpadded=True)


def fault_c0_from_c(e, sources, L):
    return _faulty(e, sources, L, c0_from_c=True)


def fault_projection_cut(e, sources, L):
    return _faulty(e, sources, L, cut=True)


# ---- the refusals of nhans_bss_eval, each by its message (no device is touched: handle may be None) ---------------------
def check_refusals(lib, handle):
    import ctypes
    from nhans_amd import context
    buf = ctypes.c_void_p(4096)             # a pointer that is never followed

    def call(est=buf, eoff=(0, 10, 20), srcs=(buf, buf), soffs=((0, 10, 20), (0, 10, 20)), n=2, L=16, out=buf):
        rc = context.bss_call(lib, handle, est, list(eoff), list(srcs), [list(o) for o in soffs], n, L, out, None, None)
        return rc, lib.nhans_last_error().decode()

    rc, msg = call(n=-1)
    assert rc == -1 and "negative clip count" in msg, msg
    rc, msg = call(srcs=(buf, buf, buf), soffs=((0, 10, 20),) * 3)
    assert rc == -1 and "3 sources" in msg, msg
    for L in (0, 513, -4):
        rc, msg = call(L=L)
        assert rc == -1 and "filter length %d" % L in msg and "1 ... 512" in msg, msg
    rc, msg = call(out=None)
    assert rc == -1 and "null" in msg, msg
    rc = lib.nhans_bss_eval(handle, buf, None, None, None, 1, 2, 16, buf, None, None)
    assert rc == -1 and "null" in lib.nhans_last_error().decode()
    rc, msg = call(eoff=(0, 10, 5))
    assert rc == -1 and "clip 1" in msg and "estimate offsets descend" in msg, msg
    rc, msg = call(soffs=((7, 3, 20), (0, 10, 20)))
    assert rc == -1 and "clip 0" in msg and "target offsets descend" in msg, msg
    rc, msg = call(soffs=((0, 10, 20), (0, 10, 9)))
    assert rc == -1 and "clip 1" in msg and "interferer offsets descend" in msg, msg
    rc, msg = call(est=None, eoff=(0, 0, 10), soffs=((0, 5, 20), (0, 5, 20)))
    assert rc == -1 and "clip 1" in msg and "null buffer" in msg, msg
    rc, msg = call(srcs=(buf, None))
    assert rc == -1 and "clip 0" in msg and "null buffer" in msg, msg
    big = 2 ** 31
    rc, msg = call(eoff=(0, 10, 10 + big), soffs=((0, 10, 10 + big), (0, 10, 10 + big)))
    assert rc == -1 and "clip 1" in msg and "%d samples" % big in msg and "2^31 - 1" in msg, msg
