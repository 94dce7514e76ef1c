"""The device-free half of tests/test_gpu_exponents.py: the helpers of tests/exponent_checks.py are fed emulated "device"
outputs built from the CPU reference (exponent_checks.Emulated: the float64 network with oracle.torch_ref's split_store /
flushed_store as storage), so that the GPU file is known to fail when it should -- and to pass on a correct device.
One tower group and one stack group carry it (a CPU pass of the tower is cheap, one of the stack is not)."""
import pytest

import nhans_amd  # noqa: F401
import layer_checks as L
import exponent_checks as X
from oracle import torch_ref as TR

KIND, RECIPE = X.CASES[0]
TOWER_GROUP, STACK_GROUP = [1, 2], [8]


@pytest.fixture(scope="module")
def yard():
    return X.Yard(KIND, RECIPE)


def _base(kind, recipe):
    return list(X.ENGINE_BASE[(kind, recipe)])


def test_ties_and_groups_agree_with_the_library():
    """host_ctx.hip, tie_exponents: tower 1-2, 3-4, 5-6; stack: block input and conv1 tensor of the channel-changing
    blocks (64 -> 128, 128 -> 256, 256 -> 512) -- the same for both models."""
    assert X.ties() == [(1, 2), (3, 4), (5, 6), (11, 12), (15, 16), (19, 20)]
    assert X.groups() == [[0], [1, 2], [3, 4], [5, 6], [7], [8], [9], [10], [11, 12], [13], [14], [15, 16], [17], [18],
                          [19, 20], [21], [22], [23], [24]]
    E = list(range(25))
    T = X.tie(E)
    assert T[1] == T[2] == 2 and T[11] == T[12] == 12 and T[19] == T[20] == 20 and T[0] == 0 and T[7] == 7 and T[24] == 24
    down = list(range(25, 0, -1))
    assert X.tie(down)[3] == X.tie(down)[4] == down[3]
    for kind, recipe in X.CASES:
        assert X.tie(X.ENGINE_BASE[(kind, recipe)]) == list(X.ENGINE_BASE[(kind, recipe)])     # what an engine reads back
    # the read-back check itself: a device that hands back other exponents than tie_exponents gives fails it
    class Deaf(X.Emulated):
        def set_exponents(self, E):
            return [0] * 25
    y = type("Y", (), {"A": [1.0] * 25})()
    f, _ = X.check_position(Deaf(None), y, [0] * 25, [1, 2], "tight", 1, "deaf")
    assert len(f) == 1 and "read back" in f[0]


def test_fetches_and_readers():
    assert X.written(0) == X.written(7) == X.written(X.EMB) == list(range(8))
    assert X.written(8) == X.written(9) == [8, 9] and X.written(12) == list(range(8, 14))
    assert X.written(24) == X.written(X.HEADS) == list(range(8, 25))
    assert X.reader([1, 2]) == 3 and X.reader([7]) is None and X.reader([23]) == 24 and X.reader([24]) is None
    assert X.fetch_list([1, 2]) == [1, 2, 3, X.EMB] and X.fetch_list([24], flat=True) == [24, 26, 27]
    assert X.quiet_before([0]) is None and X.quiet_before([8]) is None and X.quiet_before([9]) is None
    assert X.quiet_before([10]) == 9 and X.quiet_before([11, 12]) == 9 and X.quiet_before([24]) == 23
    for g in X.groups():                        # the fetch before the group really stops short of the group's writer
        q = X.quiet_before(g)
        assert q is None or max(X.written(q)) < g[0]


def test_expected_at_the_four_boundaries():
    W, F = X.LIMIT_WINO, X.LIMIT_F16
    for wino in (1, 0):
        lim = W if wino else F
        assert X.verdict_of([1.0, 0.949 * lim], wino) == "clean"
        assert X.verdict_of([1.0, 0.951 * lim], wino) == "either"
        assert X.verdict_of([0.951 * lim, 1.0], wino) == "either"
        assert X.verdict_of([1.049 * F, 1.0], wino) == "either"
        assert X.verdict_of([1.0, 1.051 * F], wino) == "flagged"
    assert X.verdict_of([0.96 * W], 1) == "either" and X.verdict_of([0.96 * W], 0) == "clean"
    assert X.verdict_of([20000.0], 1) == "either" and X.verdict_of([20000.0], 0) == "clean"
    assert X.verdict_of([], 1) == "clean"
    for a in (0.37, 4.2, 30.9, 1000.0):
        for pos, lo in X.POSITIONS.items():
            assert lo <= a * 2.0 ** -X.position_exponent(a, pos) < 2 * lo
    # and through the tensors a fetch writes: a low exponent on a tensor the fetch does not reach says nothing
    y = type("Y", (X.Yard,), {"__init__": lambda self: None})()
    y.A = [10.0] * 25
    E = [-4] * 25
    E[13] = -14                                                         # r = 163,840
    assert y.expected(12, E, 1) == "flagged" and y.expected(13, E, 1) == "flagged" and y.expected(X.HEADS, E, 1) == "flagged"
    assert y.expected(11, E, 1) == "clean" and y.expected(3, E, 1) == "clean" and y.expected(X.EMB, E, 1) == "clean"
    E[13] = -10                                                         # r = 10,240
    assert y.expected(13, E, 1) == "either" and y.expected(13, E, 0) == "clean"


def test_judge_is_check_tensor(yard):
    """exponent_checks.Yard.judge holds a tensor to the conditions of layer_checks.check_tensor / check_head with figures
    computed once: same error, same bar, same verdict."""
    for idx, shift in ((3, 0.0), (3, 1e-4), (24, 0.0), (24, 3e-4)):
        t = (yard.t64.acts[idx] + shift).float()
        v, j = L.check_tensor(idx, t, yard.t64, yard.t32, X.MODE), yard.judge(idx, t, "x")
        assert (v.ok, v.err_hip, v.bar) == (j["ok"], j["err"], j["bar"]) and v.ok == (shift == 0.0)
    for name, i, ref, c32 in (("embeddings", 25, yard.t64.emb, yard.t32.emb), ("logits", 26, yard.t64.logits, yard.t32.logits)):
        for shift in (0.0, 1e-3):
            t = (ref + shift).float()
            v, j = L.check_head(name, t, ref, c32, X.MODE), yard.judge(i, t, "x")
            assert (v.ok, v.err_hip, v.bar) == (j["ok"], j["err"], j["bar"]) and v.ok == (shift == 0.0)
    neg = yard.t64.acts[3].float().clone()
    neg[0, 0, 0, 0] = -1e-9
    assert not yard.judge(3, neg, "x")["ok"] and "post-ReLU" in yard.judge(3, neg, "x")["message"]


def test_split_storage_passes_and_the_faults_fail(yard):
    """On the tower group 1-2 (block 0's output and block 1's conv1 tensor, one exponent): a device that stores hi + lo
    f16 correctly and flags at 65504 passes tight, between, over and raised; one that clamps without the flag, and one
    that flags where everything is inside the limit, fail with a message that names tensor and position."""
    base, g = _base(KIND, RECIPE), TOWER_GROUP
    k = X.K_RAISED[(KIND, RECIPE)]
    good = X.Emulated(yard)
    for pos in ("tight", "between", "over", "raised"):
        f, rows = X.check_position(good, yard, base, g, pos, 0, "emulated", k=k if pos == "raised" else None)
        assert not f and rows, (pos, f)
    # Winograd on: `between` may be flagged or not -- unflagged, the bars hold
    f, rows = X.check_position(good, yard, base, g, "between", 1, "emulated")
    assert not f and all("either" in r for r in rows)
    silent = X.Emulated(yard, flag="never")
    f, _ = X.check_position(silent, yard, base, g, "over", 0, "emulated")
    assert len(f) == 1 and "clamped without the flag" in f[0] and "tensor 1 " in f[0] and "group [1, 2] over" in f[0], f
    for pos in ("tight", "between"):
        assert not X.check_position(silent, yard, base, g, pos, 0, "emulated")[0]
    nervous = X.Emulated(yard, flag="always")
    for pos in ("tight", "between"):
        f, _ = X.check_position(nervous, yard, base, g, pos, 0, "emulated")
        assert len(f) == len(X.fetch_list(g)) and all("raised STATUS_SATURATED" in m and "group [1, 2] " + pos in m for m in f), f
    f, _ = X.check_position(nervous, yard, base, g, "raised", 0, "emulated", k=k)
    assert f and any("tensor 3 " in m for m in f)

    # a writer that clamps below its range (here: at 60000 instead of 65504) fails `over` on the clamped elements
    class Low(X.Emulated):
        def fetch(self, i):
            t, st = super().fetch(i)
            return (t.clamp(max=60000.0 * 2.0 ** self.E[i]) if i < 25 else t), st
    f, _ = X.check_position(Low(yard), yard, base, g, "over", 0, "emulated")
    assert len(f) == 1 and "are not 65504 x 2^" in f[0], f


@pytest.mark.parametrize("kind,recipe", X.CASES)
def test_the_chosen_k_is_a_valid_flush_witness(kind, recipe):
    """k = exponent_checks.K_RAISED: on one tower group and one stack group raised by k, in float64 on the CPU, a path
    that flushes subnormal f16 halves moves the group's reader by at least 5 x (bar + 4 fmt), while bar + 4 fmt stays
    below the cap on the group's tensors and the reader -- and no smaller k of exponent_checks.KS would do (for k = 8 there
    is none)."""
    y = X.Yard(kind, recipe)
    base, k = _base(kind, recipe), X.K_RAISED[(kind, recipe)]
    assert k == X.KS[0], "a k above the smallest: add the proof that the smaller ones are not valid"
    for g in (TOWER_GROUP, STACK_GROUP):
        w = X.witness(y, base, g, k)
        print("%s %s group %s k %d: flushed moves tensor %d by %.3e = %.2f x (5 x (bar + 4 fmt)); fmt/max %s" % (
            kind, recipe, g, k, w["reader"], w["flushed"], w["flushed"] / w["need"], {j: "%.2e" % (f / y.m[j]) for j, f in w["fmt"].items()}))
        assert w["valid"] and w["capped"], (g, w["flushed"], w["need"], w["capped"])
        if (kind, recipe) != (KIND, RECIPE) or g != STACK_GROUP:
            continue
        # the GPU file's check on that output: fails at the raised position, names the reader ...
        class Flushed(X.Emulated):
            def fetch(self, i, run=w["run"]):
                t = (run[26].float(), run[27].float()) if i == X.HEADS else run[i].float()
                return t, 0
        dev = Flushed(y, store=TR.flushed_store)
        f, _ = X.check_position(dev, y, base, g, "raised", 1, "emulated flush", k=k)
        assert any("tensor %d " % w["reader"] in m and "raised by %d" % k in m for m in f), f
        # ... and passes at the base exponents, at the bar the layer tests have: today's blindness
        dev = X.Emulated(y, store=TR.flushed_store)
        dev.set_exponents(base)
        for i in X.fetch_list(g, flat=True)[:2]:
            t, st = dev.fetch(i)
            assert st == 0 and y.judge(i, t, "flushed at base")["ok"], i
