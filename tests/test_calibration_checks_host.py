"""The device-free half of tests/test_gpu_calibration.py: the conditions on the inputs the GPU file relies on, and the
proof that its checks see a fault.  tests/calibration_checks.py has the helpers; its Emulated "device" derives the maxima a
calibration bracket would record from the float64 tensors of the layer batch -- correctly, or with one of six faults of a
maximum kernel planted -- and the very check functions the GPU file runs are run on it.

Conditions (every case of calibration_checks.CASES: exponent_checks.CASES and `denoiser / one_channel_loud`):
  * no float64 maximum of the whole batch lies within its bar of a power of two: the exponent the rule must choose is
    unambiguous (the whole batch is the scope exponents are compared with float64 at; the brackets round `embed` alone and
    `activation(13)` over all frames record the same numbers);
  * every maximum at every scope -- batch, clip, frame, image -- is non-zero;
  * `one_channel_loud`: the maximum of tensor j sits in channel weight_recipes.loud_channel(j, C).
If one fails, the input changes; no tensor is exempted.

Planted faults (calibration_checks.FAULTS, (a) .. (f)): each is rejected by check_maxima or the exponent comparison at some
scope, on every case; the printed table says where (profiles/calibration/README.md keeps it).
"""
import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import spec
import layer_checks as L
import exponent_checks as X
import calibration_checks as C
import weight_recipes as R

CONFIGS_P1 = [("defaults", {}, C.F32_STORED), ("winograd_f32_tensors 0", {"winograd_f32_tensors": 0}, ()), ("winograd 0", {"winograd": 0}, ())]


@pytest.fixture(scope="module", params=C.CASES, ids=["%s-%s" % c for c in C.CASES])
def case(request):
    kind, recipe = request.param
    yard = X.Yard(kind, recipe)
    return kind, recipe, yard, C.Maxima(yard)


def run_all(dev, yard, mx, label):
    rep = C.Report(label)
    C.check_scopes(dev, yard, mx, rep)
    C.check_raise_only(dev, yard, mx, rep)
    C.check_untouched(dev, yard, mx, rep)
    for name, options, f32_stored in CONFIGS_P1:
        sub = C.Report(label)
        C.check_precision_1(dev, yard, mx, sub, options=options, f32_stored=f32_stored)
        rep.failures += sub.failures
        for k, v in sub.rejected.items():
            rep.rejected["%s, %s" % (k, name)] = v
        for k, v in sub.worst.items():
            rep.worst["%s, %s" % (k, name)] = v
    return rep


def test_rule_and_expected_exponents():
    assert C.rule(0.0) is None
    assert C.rule(1.0) == -7 and C.rule(0.999) == -8 and C.rule(255.999) == 0 and C.rule(256.0) == 1 and C.rule(128.0) == 0
    for m in (3e-5, 0.37, 4.2, 30.9, 1000.0, 65504.0):
        assert 128.0 <= m * 2.0 ** -C.rule(m) < 256.0
    prev = list(range(25))
    E = C.expected_exponents([0.0] * 25, prev)
    assert E == X.tie(prev)                                                 # nothing recorded: kept (and tied)
    m = [1.0] * 25
    assert C.expected_exponents(m, prev) == [-7] * 25
    assert C.expected_exponents(m, prev, merge=True) == X.tie(prev)         # raise only: all of prev are above -7
    m[1], m[2] = 4.0, 1000.0                                                # a tie pair: both take the larger, 1000 -> 2
    E = C.expected_exponents(m, [-9] * 25, merge=True)
    assert E[1] == E[2] == 2 and E[0] == -7
    m[3] = 0.0
    assert C.expected_exponents(m, [5] * 25)[3] == 5 and C.expected_exponents(m, [5] * 25)[4] == 5   # kept, and its partner tied up to it
    assert C.ambiguous(1.0, 1e-6) and C.ambiguous(255.9999, 1e-3) and not C.ambiguous(1.5, 1e-3) and C.ambiguous(1e-7, 1e-6)
    assert abs(C.distance_to_power_of_two(1.01) - 0.01 / 1.01) < 1e-12 and abs(C.distance_to_power_of_two(0.99) - 0.01 / 0.99) < 1e-12


def test_what_a_call_writes():
    assert C.seen(("mask_net", None)) == {j: (0, 21) for j in range(8, 25)} and C.seen(("mask_net", 1)) == {j: (11, 12) for j in range(8, 25)}
    assert C.seen(("embed", 2)) == {j: (2, 3) for j in range(8)} and C.seen(("tower_activation", 5)) == {j: (0, 3) for j in range(8)}
    assert C.seen(("activation", 13, 0, 21)) == {j: (0, 21) for j in range(8, 14)} and sorted(C.seen(("activation", 24, 20, 1))) == list(range(8, 25))
    # check_maxima: inside the bar, outside it, a tensor the bracket did not write
    want, bar = [0.0] * 8 + [2.0] * 17, [1e-5] * 25
    f, worst, at = C.check_maxima([0.0] * 8 + [2.0 + 5e-6] * 17, want, bar, scope="s", label="l")
    assert not f and abs(worst - 0.5) < 1e-6
    f, worst, at = C.check_maxima([0.0] * 8 + [2.0] * 16 + [2.0 - 3e-5], want, bar, scope="per frame [3]", label="l")
    assert len(f) == 1 and at == 24 and "tensor 24 (last_conv)" in f[0] and "per frame [3]" in f[0] and "/ bar = 3" in f[0]
    f, _, _ = C.check_maxima([0.5] + [0.0] * 7 + [2.0] * 17, want, bar, scope="s", label="l")
    assert len(f) == 1 and "tensor 0 " in f[0] and "not written" in f[0]
    f, _, _ = C.check_maxima([0.0] * 8 + [2.0 + 5e-4] * 17, want, bar, extra=C.half_extra(want, (8,)), scope="s", label="l")
    assert len(f) == 1 and "tensor 8 " in f[0]                             # (2^-11 x 2 = 9.8e-4 for the split ones)
    assert float("nan") != 0.0 and C.check_maxima([float("nan")] * 25, want, bar)[0]


def test_the_loud_recipe_is_synthetic7_with_25_channels_scaled():
    W, W7 = R.one_channel_loud("denoiser"), L.WEIGHTS["synthetic7"]("denoiser")
    scopes = R.loud_scopes()
    assert len(scopes) == 25 and [c for _, c in scopes] == [g["cout"] for g in spec.activation_geometry()]
    readers = [name for j in range(25) for name, _, _ in R.loud_readers("denoiser", j, W7)]
    assert len(readers) == len(set(readers)) and "resblock2_1_transform/w" in readers and "resblock1_2_transform/w" not in W7
    changed = sorted(k for k in W if not (W[k] == W7[k]).all())
    assert changed == sorted([s + "/" + leaf for s, _ in scopes for leaf in ("beta", "gamma")] + readers)
    up, down = 2.0 ** R.LOUD_LOG2, 2.0 ** -R.LOUD_LOG2
    for j, (s, n) in enumerate(scopes):
        c = R.loud_channel(j, n)
        assert c in (0, 31, 32, n - 1)
        for leaf in ("beta", "gamma"):
            a, b = W[s + "/" + leaf].reshape(-1), W7[s + "/" + leaf].reshape(-1)
            assert a[c] == b[c] * up and b[c] != 0 and (a != b).sum() == 1
        for name, axis, stride in R.loud_readers("denoiser", j, W7):         # that input channel, all of it, nothing else: exact
            a, b = np.moveaxis(W[name], axis, 0), np.moveaxis(W7[name], axis, 0)
            rows = np.arange(a.shape[0]) % (n if stride > 1 else a.shape[0]) == c
            assert a.shape[0] == (n * 26 if stride > 1 else n) and (a[rows] == b[rows] * down).all() and (a[~rows] == b[~rows]).all()
            assert (a[rows].astype(np.float64) * up == b[rows]).all()
    assert {R.loud_channel(j, 64) for j in range(4)} == {0, 31, 32, 63}


def test_builtin_batch_entry_point(lib_built):
    """nhans_debug_builtin_batch (host only): declared in the header's debug section and the signature table, exported;
    lengths first, then the arrays -- two trimmed 198-frame mixtures, two pairs of 200-frame context recordings, clip 1's
    first recording silent --, the same bits on every call; null lengths or some arrays missing: NHANS_EINVAL."""
    import ctypes
    import os
    import re
    from nhans_amd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nhans_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"\bint\s+nhans_debug_builtin_batch\s*\(\s*float\* mix_out, float\* ctx_a_out, float\* ctx_b_out, int64_t\* lengths_out\s*\)\s*;", code)
    assert code.index("nhans_debug_row_classes") < code.index("nhans_debug_builtin_batch") < code.index("nhans_crc32c")
    restype, argtypes = hip.SIGNATURES["nhans_debug_builtin_batch"]
    assert restype is ctypes.c_int and len(argtypes) == 4 and "nhans_debug_builtin_batch" in hip.EXPORTS
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "nhans_debug_builtin_batch") and hip.ABI_VERSION == 5
    lib = hip.load()
    n = (ctypes.c_int64 * 2)()
    assert lib.nhans_debug_builtin_batch(None, None, None, n) == 0
    assert list(n) == [spec.WIN + 197 * spec.HOP, spec.WIN + (spec.NOISE_WIN - 1) * spec.HOP] and lib.nhans_num_frames(n[0]) == 198
    buf = (ctypes.c_float * 4)()
    assert lib.nhans_debug_builtin_batch(None, None, None, None) == -1 and b"lengths" in lib.nhans_last_error()
    assert lib.nhans_debug_builtin_batch(buf, None, None, n) == -1 and lib.nhans_debug_builtin_batch(None, buf, buf, n) == -1
    assert not any(buf)
    mixes, ca, cb = hip.builtin_batch()
    again = hip.builtin_batch()
    for a, b in zip(mixes + ca + cb, again[0] + again[1] + again[2]):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert [len(a) for a in mixes] == [n[0]] * 2 and [len(a) for a in ca + cb] == [n[1]] * 4
    assert not ca[1].any() and all(a.any() and np.isfinite(a).all() for a in mixes + [ca[0]] + cb)
    # what calibrate_builtin's comment says of the signals: a voice below 0.22 x sum 1/h + noise of 0.05; the second mixture
    # 0.35 of the first plus noise of 0.12; context noises of 0.1 and 0.25 of full scale
    assert np.abs(mixes[0]).max() <= 0.22 * sum(1.0 / h for h in range(1, 13)) + 0.05
    assert np.abs(mixes[1] - np.float32(0.35) * mixes[0]).max() <= 0.12 * (1 + 1e-6) and np.abs(mixes[1] - np.float32(0.35) * mixes[0]).max() > 0.11
    assert 0.09 < np.abs(cb[0]).max() <= 0.1 and 0.24 < np.abs(cb[1]).max() <= 0.25 and np.abs(ca[0]).max() < 0.6


def test_conditions_on_the_inputs(case):
    kind, recipe, yard, mx = case
    batch = mx.batch()
    lines = []
    for j in range(25):
        assert batch[j] > 0 and batch[j] == yard.m[j]
        assert not C.ambiguous(batch[j], yard.bar[j]), (kind, recipe, j, batch[j], yard.bar[j])
        lines.append("%2d %-34s max %.6g  distance to a power of two %.2e  bar/max %.2e  exponent %d" % (
            j, L.NAMES[j], batch[j], C.distance_to_power_of_two(batch[j]), yard.bar[j] / batch[j], C.rule(batch[j])))
    print("\n%s %s\n%s" % (kind, recipe, "\n".join(lines)))
    assert min(C.distance_to_power_of_two(m) for m in batch) > 10 * max(yard.bar[j] / batch[j] for j in range(25))
    # the brackets whose exponents are compared with float64 record the whole batch's maxima of what they write
    assert mx.of([("embed", None)]) == batch[:8] + [0.0] * 17 and mx.of([("tower_activation", 3)]) == batch[:8] + [0.0] * 17
    assert mx.of([("activation", 13, 0, L.TOTAL)]) == [0.0] * 8 + batch[8:14] + [0.0] * 11
    # every checked maximum is non-zero, at every scope
    scopes = [[("mask_net", i)] for i in range(len(L.FRAMES))] + C.frame_calls() + [[("embed", i)] for i in range(L.N_CTX)]
    for calls in scopes:
        m = mx.of(calls)
        assert all(m[j] > 0 for j in C.seen(calls[0])), (kind, recipe, calls)
    if recipe == "one_channel_loud":
        for j in range(25):
            assert mx.loudest_channel(j) == R.loud_channel(j, yard.ref_cpu[j].shape[-1]), (j, mx.loudest_channel(j))
    if (kind, recipe) == ("denoiser", "synthetic7"):
        assert C.expected_exponents(batch, [0] * 25) == [-4, -4, -4, -5, -5, -5, -5, -5, -5, -5, -3, -3, -3, -4, -3, -3, -3, -4, -4, -3, -3, -3, -3, -4, -3]


def test_a_correct_device_passes_and_every_planted_fault_is_rejected(case):
    kind, recipe, yard, mx = case
    good = run_all(C.Emulated(yard, mx), yard, mx, "%s %s, emulated" % (kind, recipe))
    print("\n" + good.table())
    assert not good.failures, "\n".join(good.failures)
    lines = []
    for fault, text in C.FAULTS.items():
        rep = run_all(C.Emulated(yard, mx, fault=fault), yard, mx, "%s %s, fault (%s)" % (kind, recipe, fault))
        lines.append("(%s) %-90s rejected at: %s" % (fault, text, "; ".join("%s (%d)" % kv for kv in rep.rejected.items()) or "NOWHERE"))
        assert rep.rejected, "fault (%s) -- %s -- passes every check of the GPU file on %s %s" % (fault, text, kind, recipe)
        assert all(("tensor" in m or "exponents" in m or "bits" in m or "maximum over" in m) for m in rep.failures)
    print("\n%s %s: planted faults\n%s" % (kind, recipe, "\n".join(lines)))
