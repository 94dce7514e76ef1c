"""Shared pieces of the calibration tests (tests/test_gpu_calibration.py on the device, tests/test_calibration_checks_host.py
for the device-free half): in the split-f16 mode every stored tensor lives at a per-tensor power-of-two exponent, and the
exponents come from a calibration bracket -- option "calibrate" of include/nhans_hip.h: 1 opens it, every launch that
finishes a stored tensor then records the largest |x| of it, 0 / 2 / 3 close it (set / raise only / discard).

Everything expected here comes from the float64 reference of tests/layer_checks.py (exponent_checks.Yard: same batch, same
bar), never from the device:

  * a maximum is 1-Lipschitz in the sup norm, | max|a| - max|b| | <= max|a - b|: the bar of tensor j (Yard.bar[j], the bar
    every element of the tensor is held to) is a derived bar of its recorded maximum, at every scope -- the maximum over
    a frame, a clip or an image is a maximum over fewer of the same elements;
  * rule(): the header's rule -- "set every e so that the recorded maximum is stored as at most 2^8" -- restated from its
    text: m = f 2^k, f in [0.5, 1), e = k - 8, stored maximum in [128, 256); m == 0: the tensor keeps its exponent;
  * ambiguous(): a condition on the INPUTS -- a float64 maximum within its bar of a power of two would let two
    exponents both be right; tests/test_calibration_checks_host.py asserts that no case has one;
  * the scopes: the whole batch (one launch, and passes of 8 frames / 1 image: same bits), every clip, every one of the
    21 frames, every image.  A maximum kernel that loses the tail of a pass, the remainder of a grid-stride loop or half of
    a channel block is right at some scopes and wrong at others; FAULTS below are such kernels, emulated on the CPU, and
    the host half proves each is rejected at a scope the GPU file runs.

A `device` here is anything with exponents(), set_exponents(E) -> E read back, and

    bracket(calls, close, precision=0, options=None) -> (amax, exponents)

which opens a bracket, runs `calls` at `precision` (0: f32, 1: f16x3) with `options` (frames_per_chunk,
contexts_per_chunk, winograd, winograd_f32_tensors) off their defaults, closes it with `close` and reads both back:
the engine on the GPU, Emulated below in the host half.  A call is one of

    ("mask_net", clip or None)       the stack and head on one clip alone / the whole batch:  tensors 8 .. 24
    ("embed", image or None)         the tower on one image alone / all three:                tensors 0 .. 7
    ("activation", j, frame0, n)     nhans_debug_activation: the stack up to the block that writes tensor j
    ("tower_activation", j)          nhans_debug_tower_activation: the whole tower
"""
import math

import numpy as np

import nhans_amd  # noqa: F401
import layer_checks as L
import exponent_checks as X

TARGET_LOG2 = 8                     # "stored as at most 2^8"
CASES = list(X.CASES) + [("denoiser", "one_channel_loud")]
GRID_CAP_WORDS = 256 * 16 * 256     # words one grid of the maximum kernel covers without its stride loop
HALF_EPS = 2.0 ** -11               # a split tensor is read through its hi halves: the value rounded to 11 bits
# tensors the split-f16 mode stores as f32 NHWC in its default configuration (host_net.hip: stored_f32 -- the conv1 tensors of
# resblock1_1 / 1_2 / 2_2, the outputs of resblock1_1 / 2_1: tests/test_gpu_parity.py); none with winograd or
# winograd_f32_tensors at 0.  They are read as f32 words and owe nothing to HALF_EPS.
F32_STORED = (8, 9, 10, 13, 14)
BATCH = (("mask_net", None), ("embed", None))


# ---- the rule ----------------------------------------------------------------------------------------------------
def rule(m):
    """Exponent of a tensor whose recorded maximum is m; None: it keeps the one it has."""
    if m == 0:
        return None
    assert m > 0 and math.isfinite(m), m
    f, k = math.frexp(m)
    assert 0.5 <= f < 1 and 2.0 ** (TARGET_LOG2 - 1) <= m * 2.0 ** -(k - TARGET_LOG2) < 2.0 ** TARGET_LOG2
    return k - TARGET_LOG2


def expected_exponents(maxima, previous, merge=False):
    E = []
    for m, p in zip(maxima, previous):
        e = rule(float(m))
        E.append(p if e is None else max(p, e) if merge else e)
    return X.tie(E)


def ambiguous(m, bar):
    return not m - bar > 0 or rule(m - bar) != rule(m + bar)


def distance_to_power_of_two(m):
    """Relative distance of m to the nearest power of two."""
    f, _ = math.frexp(m)
    return min(f - 0.5, 1.0 - f) / f


# ---- what a call writes --------------------------------------------------------------------------------------------
def seen(call):
    """{tensor: (first, end)} -- the frames (stack) / images (tower) of the layer batch whose tensors the call finishes."""
    what = call[0]
    if what == "mask_net":
        lo, hi = (0, L.TOTAL) if call[1] is None else (L.FOFF[call[1]], L.FOFF[call[1] + 1])
        return {j: (lo, hi) for j in L.STACK_IDX}
    if what == "embed":
        lo, hi = (0, L.N_CTX) if call[1] is None else (call[1], call[1] + 1)
        return {j: (lo, hi) for j in L.TOWER_IDX}
    if what == "activation":
        _, j, g0, n = call
        return {t: (g0, g0 + n) for t in X.written(j)}
    if what == "tower_activation":
        return {j: (0, L.N_CTX) for j in L.TOWER_IDX}
    raise KeyError(call)


class Maxima:
    """max|x| of the float64 tensors of a Yard per frame / image and channel -- pf[j]: [N, C] -- and over what a list of
    calls writes."""

    def __init__(self, yard):
        self.yard = yard
        self.pf = {j: yard.ref_cpu[j].abs().amax(dim=(1, 2)) for j in range(25)}

    def of(self, calls):
        m = [0.0] * 25
        for call in calls:
            for j, (lo, hi) in seen(call).items():
                m[j] = max(m[j], float(self.pf[j][lo:hi].max()))
        return m

    def batch(self):
        return self.of(BATCH)

    def loudest_channel(self, j):
        return int(self.pf[j].amax(dim=0).argmax())


# ---- the comparison --------------------------------------------------------------------------------------------------
def check_maxima(got, want, bar, extra=None, scope="", label=""):
    """|got_j - want_j| <= bar_j + extra_j for every tensor the bracket recorded (want_j > 0); a tensor it did not write
    reports 0 -- a bracket starts from zero maxima.  -> (failures, worst ratio to the bar, its tensor)."""
    failures, worst, at = [], 0.0, None
    for j in range(25):
        g, w = float(got[j]), float(want[j])
        if w == 0.0:
            if g != 0.0:
                failures.append("%s, %s: tensor %d (%s) is not written inside this bracket and reports a maximum of %.6g" % (
                    label, scope, j, L.NAMES[j], g))
            continue
        b = bar[j] + (extra[j] if extra else 0.0)
        ratio = abs(g - w) / b if math.isfinite(g) else float("inf")
        if ratio > worst:
            worst, at = ratio, j
        if not ratio <= 1.0:
            failures.append("%s, %s: tensor %d (%s): recorded maximum %.9g, float64 %.9g: |difference| / bar = %.3g (bar %.3e%s)" % (
                label, scope, j, L.NAMES[j], g, w, ratio, bar[j], " + %.3e for the hi halves" % extra[j] if extra and extra[j] else ""))
    return failures, worst, at


def half_extra(want, f32_stored=()):
    """The derived allowance of a bracket at precision 1: 2^-11 of the maximum for the tensors read through hi halves."""
    return [0.0 if j in f32_stored else HALF_EPS * want[j] for j in range(25)]


class Report:
    """Failures, the printed rows and the worst ratio per scope of one run of checks."""

    def __init__(self, label):
        self.label, self.failures, self.rows, self.worst, self.rejected = label, [], [], {}, {}

    def add(self, scope, failures, worst=None, at=None):
        self.failures += failures
        if failures:
            self.rejected[scope.split(" [")[0]] = self.rejected.get(scope.split(" [")[0], 0) + len(failures)
        if worst is not None:
            key = scope.split(" [")[0]
            if worst >= self.worst.get(key, (-1.0, None))[0]:
                self.worst[key] = (worst, at)

    def table(self):
        return "\n".join("%-44s %-34s worst |amax - f64 max| / bar %.4f at tensor %s" % (self.label, k, w, a)
                         for k, (w, a) in self.worst.items())


def check_bracket(dev, yard, mx, calls, scope, rep, close=0, precision=0, options=None, f32_stored=(), vs_f64=True):
    """One bracket round `calls`: recorded maxima against float64; exponents against the rule applied to the float64
    maxima (vs_f64; where `scope` is one whose maxima are known unambiguous) and -- exactly, always -- to the maxima as
    reported; tie pairs equal.  -> (amax, exponents)."""
    prev = dev.exponents()
    amax, E = dev.bracket(calls, close, precision=precision, options=options)
    want = mx.of(calls)
    if close == 3:
        if E != prev:
            rep.add(scope, ["%s, %s: closed with 3 (discard), exponents moved: %s -> %s" % (rep.label, scope, prev, E)])
        return amax, E
    extra = half_extra(want, f32_stored) if precision else None
    f, worst, at = check_maxima(amax, want, yard.bar, extra, scope, rep.label)
    rep.add(scope, f, worst, at)
    problems = []
    finite = all(math.isfinite(float(a)) and a >= 0 for a in amax)
    if finite and E != expected_exponents(amax, prev, merge=close == 2):
        problems.append("exponents %s are not the rule applied to the reported maxima, %s" % (E, expected_exponents(amax, prev, merge=close == 2)))
    if vs_f64 and E != expected_exponents(want, prev, merge=close == 2):
        problems.append("exponents %s are not the rule applied to the float64 maxima, %s (before the bracket: %s)" % (
            E, expected_exponents(want, prev, merge=close == 2), prev))
    for i, j in X.ties():
        if E[i] != E[j]:
            problems.append("tensors %d and %d feed one accumulator and carry exponents %d and %d" % (i, j, E[i], E[j]))
    rep.add(scope, ["%s, %s: %s" % (rep.label, scope, p) for p in problems])
    return amax, E


# ---- the checks both halves run ------------------------------------------------------------------------------------
def frame_calls():
    return [[("activation", 24, g, 1)] for g in range(L.TOTAL)]


def check_scopes(dev, yard, mx, rep):
    """Maxima against float64 at precision 0: whole batch in one launch, the same in passes (same bits), per clip, per
    frame, per image; the maximum over the frames / images is the whole batch's, bit for bit."""
    base = dev.exponents()
    try:
        whole, _ = check_bracket(dev, yard, mx, BATCH, "whole batch, one launch", rep)
        dev.set_exponents(base)
        chunked, _ = check_bracket(dev, yard, mx, BATCH, "whole batch, passes of 8 frames and 1 image", rep,
                                   options={"frames_per_chunk": L.CHUNK, "contexts_per_chunk": 1})
        if list(chunked) != list(whole):
            rep.add("whole batch, passes of 8 frames and 1 image", ["%s: passes of %d frames / 1 image record other bits than one launch: %s" % (
                rep.label, L.CHUNK, [(j, whole[j], chunked[j]) for j in range(25) if whole[j] != chunked[j]])])
        for i in range(len(L.FRAMES)):
            dev.set_exponents(base)
            check_bracket(dev, yard, mx, [("mask_net", i)], "per clip [%d]" % i, rep, vs_f64=False)
        over = [0.0] * 25
        for g, calls in enumerate(frame_calls()):
            dev.set_exponents(base)
            a, _ = check_bracket(dev, yard, mx, calls, "per frame [%d]" % g, rep, vs_f64=False)
            over = [max(o, float(x)) if math.isfinite(float(x)) else x for o, x in zip(over, a)]
        for i in range(L.N_CTX):
            dev.set_exponents(base)
            a, _ = check_bracket(dev, yard, mx, [("embed", i)], "per image [%d]" % i, rep, vs_f64=False)
            over = [max(o, float(x)) if math.isfinite(float(x)) else x for o, x in zip(over, a)]
        if list(over) != list(whole):
            rep.add("maximum over frames and images", ["%s: the maximum over the per-frame and per-image brackets is not the whole batch's: %s" % (
                rep.label, [(j, whole[j], over[j]) for j in range(25) if whole[j] != over[j]])])
    finally:
        dev.set_exponents(base)


def check_raise_only(dev, yard, mx, rep):
    """Exponents at the float64 rule's values -2 / +2 alternating (a tie pair's members move in opposite directions), read
    back; a bracket at precision 0 closed with 2 gives the rule merged with what was read back."""
    base = dev.exponents()
    try:
        E0 = expected_exponents(mx.batch(), [0] * 25)
        start = dev.set_exponents([e + (2 if j % 2 else -2) for j, e in enumerate(E0)])
        if start != X.tie([e + (2 if j % 2 else -2) for j, e in enumerate(E0)]):
            rep.add("raise only", ["%s: exponents read back %s" % (rep.label, start)])
        assert any(start[j] != E0[j] - 2 for _, j in X.ties())       # (a tie changed what was set: its members moved apart)
        check_bracket(dev, yard, mx, BATCH, "raise only", rep, close=2)
    finally:
        dev.set_exponents(base)


def check_untouched(dev, yard, mx, rep):
    """A tensor a bracket does not write keeps its exponent -- starting from exponents 3 above the rule's, so that "kept"
    and "calibrated" differ --; a bracket closed with 3 moves none; the next bracket starts from zero maxima."""
    base = dev.exponents()
    try:
        E0 = expected_exponents(mx.batch(), [0] * 25)
        for calls, scope in (([("embed", None)], "embed only"), ([("activation", 13, 0, L.TOTAL)], "activation 13 only")):
            dev.set_exponents([e + 3 for e in E0])
            _, E = check_bracket(dev, yard, mx, calls, scope, rep)
            written = set(seen(calls[0]))
            written |= {k for t in X.ties() if written & set(t) for k in t}         # (a written tensor's tie partner follows it)
            moved = [j for j in range(25) if j not in written and E[j] != E0[j] + 3]
            if moved:
                rep.add(scope, ["%s, %s: tensors %s are not written and changed their exponents" % (rep.label, scope, moved)])
        dev.set_exponents([e + 3 for e in E0])
        check_bracket(dev, yard, mx, BATCH, "discarded", rep, close=3)              # the loud bracket ...
        check_bracket(dev, yard, mx, [("mask_net", 1)], "quiet after loud", rep, vs_f64=False)     # ... then the one-frame clip
    finally:
        dev.set_exponents(base)


def check_precision_1(dev, yard, mx, rep, options=None, f32_stored=()):
    """A bracket at precision 1 at the exponents in effect: every maximum within bar + 2^-11 max (split tensors)."""
    base = dev.exponents()
    try:
        check_bracket(dev, yard, mx, BATCH, "precision 1", rep, precision=1, options=options, f32_stored=f32_stored, vs_f64=False)
    finally:
        dev.set_exponents(base)


# ---- an emulated device, from the CPU reference ------------------------------------------------------------------
FAULTS = {
    "a": "the last frame of a pass is not seen",
    "b": "only the first 256 x 16 x 256 words of a tensor are seen (the grid cap without the stride loop)",
    "c": "channels >= 32 of each 64-half block are not seen",
    "d": "the second tensor of a tie pair is not seen",
    "e": "the maxima of the previous bracket are not cleared",
    "f": "an f32-stored tensor is read as half pairs",
}


class Emulated:
    """What a device would report if its maximum kernel had `fault` (None: a correct one): maxima derived from the
    float64 tensors, exponents by rule()."""

    def __init__(self, yard, mx, fault=None, exponents=None):
        self.yard, self.mx, self.fault = yard, mx, fault
        self.E = X.tie(exponents if exponents is not None else expected_exponents(mx.batch(), [0] * 25))
        self.running = [0.0] * 25
        self.amax = [0.0] * 25
        self.last_status = 0

    def exponents(self):
        return list(self.E)

    def set_exponents(self, E):
        self.E = X.tie(E)
        return list(self.E)

    def _pass(self, j, p0, p1, precision, f32_stored):
        """What the kernel reports of tensor j's frames / images [p0, p1): one launch."""
        fault, ref = self.fault, self.yard.ref_cpu[j]
        if fault == "d" and any(j == t[1] for t in X.ties()):
            return 0.0
        if fault == "a":
            p1 -= 1
            if p1 <= p0:
                return 0.0
        scale = 2.0 ** self.E[j]
        if fault == "f" and precision and j in f32_stored:
            halves = (ref[p0:p1] / scale).float().numpy().reshape(-1).view(np.float16)
            with np.errstate(invalid="ignore"):
                m = float("nan") if np.isnan(halves).any() else float(np.abs(halves).max())
            return m * scale
        if fault == "b":
            m = float(ref[p0:p1].reshape(-1)[:GRID_CAP_WORDS].abs().max())
        elif fault == "c":
            C = ref.shape[-1]
            keep = [c for c in range(C) if c % 64 < 32]
            m = float(self.mx.pf[j][p0:p1][:, keep].max())
        else:
            m = float(self.mx.pf[j][p0:p1].max())
        if precision and j not in f32_stored:           # the hi halves of the stored values
            m = float(np.float16(m / scale)) * scale
        return m

    def bracket(self, calls, close, precision=0, options=None):
        options = options or {}
        f32_stored = F32_STORED if precision and options.get("winograd", 1) and options.get("winograd_f32_tensors", 1) else ()
        if self.fault != "e":
            self.running = [0.0] * 25
        for call in calls:
            for j, (lo, hi) in seen(call).items():
                step = options.get("frames_per_chunk", 3776) if j >= 8 else options.get("contexts_per_chunk", 64)
                for p0 in range(lo, hi, step):
                    m = self._pass(j, p0, min(p0 + step, hi), precision, f32_stored)
                    self.running[j] = m if m != m or m > self.running[j] else self.running[j]
        if close == 3:
            return list(self.amax), list(self.E)
        run32 = [float(np.float32(m)) for m in self.running]
        if all(math.isfinite(m) for m in run32):
            self.amax = run32
            self.E = expected_exponents(run32, self.E, merge=close == 2)
            return list(self.amax), list(self.E)
        if close == 2:                                  # (non-finite maxima are skipped by the raise-only close)
            keep = [m if math.isfinite(m) else 0.0 for m in run32]
            self.E = expected_exponents(keep, self.E, merge=True)
        return run32, list(self.E)                      # (a device refuses to close with 0 here; the garbage is what matters)
