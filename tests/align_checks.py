"""What tests/test_align_host.py and tests/test_gpu_align.py share: the clips, the float64 bars and the planted faults.

The bars.  U = 2^-53.  The reference (nhans_amd.score.align_reference) rounds every sum once (math.fsum of the exact
products); the device (align.hip) adds the same exact products in a fixed order of its own.
  * c[d].  m_d = the overlap count of lag d, A_d = sum_u |e[u + d] t[u]|.  A sum of m exact terms added one after the other
    in ANY order takes m - 1 roundings, each at most U times a partial sum that is itself at most A_d: off by at most
    (m_d - 1) U A_d, plus U A_d for the reference's one rounding:  bar_c[d] = m_d U A_d.  It is 0 where m_d <= 1 -- such a
    value is exact on both sides.
  * rho = c_peak / sqrt(See Stt).  See and Stt are sums of ne and nt exact squares: relative error (ne + nt) U / 2 under the
    root with the sums, 1.5 U for the product and the root, U for the quotient, twice (either side):
        bar_rho = |rho| (bar_c[delay] / |c_peak| + (ne + nt + 6) U).
  * The delay has no bar: it must be EQUAL on every clip, and `delay_is_decided` asserts on the reference alone why it can
    be: either the winning lag leads every other lag by more than twice the largest bar of the clip (then no rounding on
    either side changes the order), or the clip is an EXACT clip -- integer samples of |x| <= 1024, whose products and sums
    are integers below 2^53 -- for which every c[d] of the device must equal the reference bit for bit, ties included.
The worst measured ratios are in profiles/align/README.md; a ratio above one half would be a defect to find.

Shapes.  TS and LB mirror align.hip's sample tile and lag block (test_align_host.py holds them to the kernel's text).
Every n of {0, 1, 2, TS - 1, TS, TS + 1, 2 TS + 3, ~16000} with ne != nt in both directions, every D of {0, 1, LB - 1, LB,
LB + 1, 2 LB + 1} and 16000, the true delay at -D, +D, 0 and beyond D, D > n (lags with empty ranges), and one clip of
two tiles across three lag blocks.  The cost of the reference is the sum of the overlaps, about (2 D + 1) n where n > D and
ne nt where D > n: the shapes pair a large D with a small n and keep the whole list to seconds.

Planted faults (test_align_host.py): each must leave the bar by orders of magnitude, so the bar is known to see them."""
import functools
import math

import numpy as np

from nhans_amd import hip, score

U = 2.0 ** -53
TS, LB = hip.ALIGN_TILE, hip.ALIGN_LAG_BLOCK
assert (TS, LB) == (2048, 2048)

# (ne, nt, D, true delay, exact)
SHAPES = [
    (0, 0, 1, 0, True), (0, 5, 3, 0, True), (5, 0, 3, 0, True), (1, 1, 0, 0, True), (1, 2, 2, 1, True), (2, 1, 1, -1, True),
    (2, 2, LB - 1, 0, True),                                # D > n: most lags have empty ranges
    (TS - 1, TS + 40, 1, 1, False),                         # the delay at +D
    (TS + 30, TS, 1, -1, False),                            # the delay at -D
    (TS + 1, TS - 5, 0, 0, False),                          # D = 0
    (TS + 8, TS + 1, LB + 1, 0, False),                     # two tiles across three lag blocks
    (2 * TS + 3, 2 * TS + 53, 300, 500, False),             # the true delay beyond D
    (2500, 2600, LB, LB, False),                            # +D at a block's edge
    (2300, 2400, LB - 1, -(LB - 1), False),                 # -D
    (400, 390, 2 * LB + 1, -100, False),                    # D > n, five lag blocks
    (2000, 2010, 16000, 700, False),                        # the largest D
    (16000, 15990, 100, 37, False),
    (15990, 16001, 100, -64, False),
]
# the exact clips of the issue: (estimate's ones at, target's ones at, n, D, delay)
TIE_CLIPS = [((2, 8), (5,), 12, 6, 3), ((4, 8), (5,), 12, 6, -1), ((), (5,), 12, 6, 0)]


# ---- clips ----------------------------------------------------------------------------------------
def delayed_pair(ne, nt, delay, seed, noise=0.5):
    """-> (e [ne], t [nt]) float32: white noise t at speech-like level and a copy of the same signal `delay` samples late
    (e[u + delay] = t[u] wherever both exist) plus white noise at `noise` times its level"""
    rng = np.random.default_rng(5000 + seed)
    p = max(delay, 0)
    s = 0.1 * rng.standard_normal(max(p + nt, p - delay + ne) + 1)
    t = s[p:p + nt]
    e = s[p - delay:p - delay + ne] + noise * 0.1 * rng.standard_normal(ne)
    return e.astype(np.float32), t.astype(np.float32)


def exact_pair(ne, nt, delay, seed):
    """the same with integer samples of |x| <= 1024 and integer noise: every product and every sum is exact"""
    rng = np.random.default_rng(6000 + seed)
    p = max(delay, 0)
    s = rng.integers(-700, 701, max(p + nt, p - delay + ne) + 1)
    t = s[p:p + nt]
    e = s[p - delay:p - delay + ne] + rng.integers(-300, 301, ne)
    assert max([0] + np.abs(e).tolist() + np.abs(t).tolist()) <= 1024
    return e.astype(np.float32), t.astype(np.float32)


def shape_clip(i):
    ne, nt, D, delay, exact = SHAPES[i]
    return (exact_pair if exact else delayed_pair)(ne, nt, delay, i)


def tie_clip(k):
    eo, to, n, D, delay = TIE_CLIPS[k]
    e, t = np.zeros(n, np.float32), np.zeros(n, np.float32)
    e[list(eo)] = 1.0
    t[list(to)] = 1.0
    return e, t


def is_exact(e, t):
    both = np.concatenate([np.asarray(e, np.float64), np.asarray(t, np.float64)])
    return bool(np.all(both == np.rint(both)) and np.all(np.abs(both) <= 1024))


# ---- the bars -------------------------------------------------------------------------------------
def corr_bars(e, t, D):
    """-> float64 [2 D + 1]: bar_c[d] = m_d U sum_u |e[u + d] t[u]|"""
    e, t = np.abs(np.asarray(e, np.float32).astype(np.float64)), np.abs(np.asarray(t, np.float32).astype(np.float64))
    out = np.zeros(2 * D + 1)
    for d in range(-D, D + 1):
        lo, hi = max(0, -d), min(len(t), len(e) - d)
        if hi - lo > 1:
            out[d + D] = (hi - lo) * U * float(np.dot(e[lo + d:hi + d], t[lo:hi])) * (1.0 + 2.0 ** -40)   # (the dot itself rounds)
    return out


def rho_bar(ref, bars):
    if not math.isfinite(ref["rho"]) or ref["c_peak"] == 0.0:
        return 0.0
    return abs(ref["rho"]) * (bars[ref["delay"] + ref["D"]] / abs(ref["c_peak"]) + (ref["ne"] + ref["nt"] + 6) * U)


def delay_is_decided(e, t, ref, bars):
    """Asserts, on the reference alone, that the clip's delay can be held to equality (see the head of the file) -> "exact"
    or the winner's least lead over another lag in units of the largest bar."""
    if is_exact(e, t):
        return "exact"
    c, D, w = ref["corr"], ref["D"], ref["delay"]
    others = np.delete(c, w + D)
    if not len(others):
        return math.inf
    lead, big = float(c[w + D] - others.max()), float(bars.max())
    assert lead > 2.0 * big, "the winning lag %d leads by %.3e, the largest bar is %.3e" % (w, lead, big)
    return lead / big if big > 0 else math.inf


@functools.lru_cache(maxsize=None)
def shape_reference(i):
    """-> (e, t, reference record with "corr", bars, how the delay is decided), computed once per session"""
    e, t = shape_clip(i)
    D = SHAPES[i][2]
    ref = score.align_reference(e, t, D, corr=True)
    bars = corr_bars(e, t, D)
    return e, t, ref, bars, delay_is_decided(e, t, ref, bars)


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


def align_ratios(rec, corr, e, t, ref, bars):
    """rec: dict by score.ALIGN_FIELDS, corr: float64 [2 D + 1] -> {"corr": the worst ratio of a lag to its bar, "rho": rho's};
    the counts and the delay must be equal, c_peak must be the lag vector's own value, and an exact clip's lag vector must
    be the reference's bit for bit."""
    for k in ("ne", "nt", "D", "delay", "n_common"):
        assert int(rec[k]) == ref[k], (k, rec[k], ref[k])
    D = ref["D"]
    assert same_bits(rec["c_peak"], corr[ref["delay"] + D])
    if is_exact(e, t):
        assert same_bits(corr, ref["corr"]), "an exact clip's lag vector differs from the reference"
    diff = np.abs(np.asarray(corr, np.float64) - ref["corr"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0.0, 0.0, np.where(bars > 0, diff / bars, np.inf))
    return {"corr": float(r.max()), "rho": ratio(rec["rho"], ref["rho"], rho_bar(ref, bars))}


# ---- the device's own order on the host ----------------------------------------------------------------
def device_order_corr(e, t, D):
    """The lag vector in the order align.hip states -- tiles of TS samples anchored at the target's u = 0; a tile's part one
    chain from +0.0 over its u ascending; the parts added ascending from +0.0 -- float64 [2 D + 1].  The products are exact,
    so a fused multiply-add is a plain addition of the product and numpy's sequential cumsum is that chain: the result is
    what the device must give bit for bit."""
    e, t = np.asarray(e, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    out = np.zeros(2 * D + 1)
    for d in range(-D, D + 1):
        lo, hi = max(0, -d), min(len(t), len(e) - d)
        c = 0.0
        for k in range(lo // TS, -(-hi // TS) if hi > lo else 0):
            a, b = max(lo, k * TS), min(hi, (k + 1) * TS)
            c = c + float(np.cumsum(e[a + d:b + d] * t[a:b])[-1])
        out[d + D] = c
    return out


# ---- planted faults: the definition put together wrongly -> (record, lag vector) ---------------------
def _record(e, t, D, c, pick=score.align_pick):
    d = pick(c, D)
    See, Stt = score._fsum((e.astype(np.float64) ** 2).tolist()), score._fsum((t.astype(np.float64) ** 2).tolist())
    with np.errstate(all="ignore"):
        rho = float(np.float64(c[d + D]) / np.sqrt(np.float64(See) * np.float64(Stt)))
    return {"ne": len(e), "nt": len(t), "D": D, "delay": d, "c_peak": float(c[d + D]), "rho": rho,
            "n_common": score.align_common(len(e), len(t), d)}, c


def fault_sample_dropped_at_tile_edge(e, t, D):
    """the first sample of the target's second tile is passed over"""
    assert len(t) > TS
    t2 = np.array(t, np.float32)
    t2[TS] = 0.0
    return _record(e, t, D, score.align_reference(e, t2, D, corr=True)["corr"])


def fault_lag_table_off_by_one(e, t, D):
    """c[d] holds the sum of lag d + 1"""
    c = score.align_reference(e, t, D + 1, corr=True)["corr"]
    return _record(e, t, D, c[2:].copy())


def fault_swapped(e, t, D):
    """the estimate and the target change places: the lag vector is mirrored"""
    c = score.align_reference(t, e, D, corr=True)["corr"]
    return _record(e, t, D, c.copy())


def reversed_pick(c, D):
    """the tie rule the wrong way round: of equal values the larger |d|, the negative one"""
    best = -D
    for d in sorted(range(-D, D + 1), key=lambda d: (-abs(d), d)):
        if c[d + D] > c[best + D]:
            best = d
    return best


def fault_tie_rule_reversed(e, t, D):
    return _record(e, t, D, score.align_reference(e, t, D, corr=True)["corr"], pick=reversed_pick)


# ---- the refusals of nhans_align and nhans_align_cut, each by its message (no device is touched: handle may be None) --------
def check_refusals(lib, handle, buf=None, out=None):
    """buf / out: device pointers the calls must leave alone (the GPU test passes guarded buffers and looks at them
    afterwards); by default a pointer that is never followed."""
    import ctypes
    buf = buf if buf is not None else ctypes.c_void_p(4096)
    out = out if out is not None else ctypes.c_void_p(8192)
    i64 = hip.i64_array

    def align(est=buf, eoff=(0, 10, 20), tgt=buf, toff=(0, 10, 20), n=2, D=16, rec=out, corr=None):
        rc = lib.nhans_align(handle, est, i64(eoff) if eoff is not None else None, tgt, i64(toff) if toff is not None else None, n, D,
                             rec, corr, None)
        return rc, lib.nhans_last_error().decode()

    def cut(est=buf, eoff=(0, 10, 20), tgt=buf, toff=(0, 10, 20), n=2, delays=(1, -1), eo=out, to=out, ooff=(0, 9, 18)):
        rc = lib.nhans_align_cut(handle, est, i64(eoff) if eoff is not None else None, tgt, i64(toff) if toff is not None else None, n,
                                 i64(delays) if delays is not None else None, eo, to, i64(ooff) if ooff is not None else None, None)
        return rc, lib.nhans_last_error().decode()

    rc, msg = align(n=-1)
    assert rc == -1 and "negative clip count" in msg, msg
    for D in (-1, 16001, 1 << 20):
        rc, msg = align(D=D)
        assert rc == -1 and "max_lag %d" % D in msg and "0 ... 16000" in msg, msg
    for kw in ({"rec": None}, {"eoff": None}, {"toff": None}):
        rc, msg = align(**kw)
        assert rc == -1 and "null" in msg, msg
    rc, msg = align(eoff=(0, 10, 5))
    assert rc == -1 and "clip 1" in msg and "estimate offsets descend" in msg, msg
    rc, msg = align(toff=(7, 3, 20))
    assert rc == -1 and "clip 0" in msg and "target offsets descend" in msg, msg
    rc, msg = align(est=None, eoff=(0, 0, 10))
    assert rc == -1 and "clip 1" in msg and "null buffer" in msg, msg
    rc, msg = align(tgt=None)
    assert rc == -1 and "clip 0" in msg and "null buffer" in msg, msg
    big = 2 ** 31
    rc, msg = align(toff=(0, 10, 10 + big))
    assert rc == -1 and "clip 1" in msg and "%d samples" % big in msg and "2^31 - 1" in msg, msg

    rc, msg = cut(n=-1)
    assert rc == -1 and "negative clip count" in msg, msg
    for kw in ({"eoff": None}, {"toff": None}, {"delays": None}, {"ooff": None}):
        rc, msg = cut(**kw)
        assert rc == -1 and "null" in msg, msg
    for kw in ({"est": None}, {"eo": None}, {"tgt": None}, {"to": None}):
        rc, msg = cut(**kw)
        assert rc == -1 and "null" in msg and "pair" in msg, msg
    rc, msg = cut(eoff=(0, 10, 5))
    assert rc == -1 and "clip 1" in msg and "estimate offsets descend" in msg, msg
    rc, msg = cut(toff=(0, 10, 9))
    assert rc == -1 and "clip 1" in msg and "target offsets descend" in msg, msg
    rc, msg = cut(ooff=(5, 2, 30))
    assert rc == -1 and "clip 0" in msg and "output offsets descend" in msg, msg
    rc, msg = cut(delays=(1, 11))
    assert rc == -1 and "clip 1" in msg and "delay 11" in msg and "10 samples of the estimate" in msg, msg
    rc, msg = cut(delays=(-12, 0), toff=(0, 11, 20))
    assert rc == -1 and "clip 0" in msg and "delay -12" in msg and "11 samples of the target" in msg, msg
    rc, msg = cut(ooff=(0, 9, 17))
    assert rc == -1 and "clip 1" in msg and "output room" in msg and "8 samples, 9 needed" in msg, msg
    assert lib.nhans_align_common(10, 10, 1) == 9 and lib.nhans_align_common(10, 12, -3) == 9
    assert lib.nhans_align_common(5, 5, 9) == 0 and lib.nhans_align_common(0, 7, 0) == 0
