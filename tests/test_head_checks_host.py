"""CPU half of tests/test_gpu_heads.py and of the head verdicts of tests/test_gpu_layers.py: the checks themselves under
test (layer_checks.check_head, tests/head_checks.py).

  * the yardstick conditions of every case whose reference can be computed without the device: float32 CPU against
    float64 within CAP x max, and the bar of either mode below CAP x max -- conditions on the references alone;
  * the faults planted in last_dense/w are valid witnesses; the pool's faults (it has no weights) and a stray store
    behind an output buffer are caught, by name.
"""
import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
import head_checks as H
import layer_checks as L


def _conditions(name, r64, r32, label):
    """check_head with the float32 CPU restatement in the device's place: ok == both yardstick conditions hold."""
    out = []
    for mode in L.BAR:
        v = L.check_head(name, r32, r64, r32, mode, label)
        assert v.ok, v.message
        assert v.err_cpu32 <= L.CAP * v.m and v.bar < L.CAP * v.m, v.row()
        out.append(v)
    return out


# (denoiser synthetic7 last: the tests below continue from the cached reference)
@pytest.mark.parametrize("kind,recipe", [(k, r) for k in ("separator", "denoiser") for r in ("heavy", "trained_bn", "synthetic7")])
def test_yardstick_conditions_of_the_heads_on_the_layer_batch(kind, recipe):
    W, lms, ctx, emb_in, t64, t32 = L.reference(kind, recipe)
    assert float((t64.denoised - (torch.from_numpy(np.concatenate(lms)).double() + t64.logits)).abs().max()) == 0.0
    for name, r64, r32 in (("embeddings", t64.emb, t32.emb), ("logits", t64.logits, t32.logits), ("denoised", t64.denoised, t32.denoised)):
        for v in _conditions(name, r64, r32, "%s %s" % (kind, recipe)):
            print(v.row())


def test_yardstick_conditions_of_the_isolated_heads():
    """The float32 CPU tensors 24 and 7 stand in for the device's taps; both float32 yardsticks (torch's order, the
    kernel's documented order) meet the conditions, and the kernel-order restatement itself is inside the bar."""
    W, lms, ctx, emb_in, t64, t32 = L.reference(L.FAULT_KIND, L.FAULT_RECIPE)
    centre = torch.from_numpy(np.concatenate(lms))
    d = H.dense_refs(t32.acts[24], W, centre)
    for which, name in enumerate(("logits", "denoised")):
        for key in ("cpu32", "cpu32_grouped"):
            for v in _conditions(name, d["f64"][which], d[key][which], "isolated dense head, yardstick " + key):
                print(key, v.row())
        for mode in L.BAR:
            v = L.check_head(name, d["cpu32_grouped"][which], d["f64"][which], d["cpu32"][which], mode, "32 K-groups in float32")
            assert v.ok, v.message
    # one frame alone (T = 1) and the one-frame clip's row: the conditions hold row by row too
    for r in (0, 11, 20):
        one = H.dense_refs(t32.acts[24][r:r + 1], W, centre[r:r + 1])
        for which, name in enumerate(("logits", "denoised")):
            _conditions(name, one["f64"][which], one["cpu32"][which], "isolated dense head, frame %d alone" % r)
    p = H.pool_refs(t32.acts[7])
    for key in ("cpu32", "cpu32_kernel_order"):
        for v in _conditions("embeddings", p["f64"], p[key], "isolated pool head, yardstick " + key):
            print(key, v.row())
    for mode in L.BAR:
        v = L.check_head("embeddings", p["cpu32_kernel_order"], p["f64"], p["cpu32"], mode, "4 interleaved sums in float32")
        assert v.ok, v.message
    # the constant image alone (n = 1)
    one = H.pool_refs(t32.acts[7][1:2])
    _conditions("embeddings", one["f64"], one["cpu32"], "isolated pool head, the constant ln 1e-5 image alone")


def test_yardstick_conditions_of_the_one_hot_case(weights_denoiser):
    t64 = H.onehot_taps(weights_denoiser, "denoiser", torch.float64)
    t32 = H.onehot_taps(weights_denoiser, "denoiser", torch.float32)
    for idx in H.ONEHOT_TENSORS:
        for mode in L.BAR:
            v = L.check_tensor(idx, t32.acts[idx], t64, t32, mode, "one-hot embeddings")
            assert v.ok, v.message
    for name, r64, r32 in (("logits", t64.logits, t32.logits), ("denoised", t64.denoised, t32.denoised)):
        _conditions(name, r64, r32, "one-hot embeddings")
    ea, eb = H.onehot_embeddings()
    assert H.onehot_logmag().shape == (4, H.BINS)
    assert sorted(map(tuple, np.argwhere(ea))) == [(1, 0), (2, 511)] and sorted(map(tuple, np.argwhere(eb))) == [(2, 256), (3, 511)]
    # the picked rows of cond.w are what the case sees: against the same four frames with all-zero embeddings, clip 0 is
    # unchanged and every other clip moves each tensor and the logits by more than 100 x the bar
    z64 = H.onehot_taps(weights_denoiser, "denoiser", torch.float64, (np.zeros_like(ea), np.zeros_like(eb)))
    K, F = max(L.BAR.values())
    for what, a, z, a32 in [(str(i), t64.acts[i], z64.acts[i], t32.acts[i]) for i in H.ONEHOT_TENSORS] + [("logits", t64.logits, z64.logits, t32.logits)]:
        bar = K * float((a32.double() - a).abs().max()) + F * float(a.abs().max())
        assert torch.equal(a[0], z[0]), what
        for clip in (1, 2, 3):
            assert float((a[clip] - z[clip]).abs().max()) > 100 * bar, (what, clip, float((a[clip] - z[clip]).abs().max()), bar)


def test_planted_head_faults_are_valid_witnesses():
    """A slice of last_dense/w rounded to f16 is a valid witness of what check_head adds at the logits if, in float64 on
    the layer tests' batch, it (1) changes no weight any tensor up to 24 depends on, (2) moves the logits by less than the
    LOGIT_TOL bar the suite had before and (3) by at least five times check_head's bar of either mode, which stays below
    the cap; the one-bin fault moves exactly bin 200.  The bar of (3) is the isolated head's with the float32 yardstick
    summed elementwise in the kernel's documented order (head_checks.HEAD_FAULTS says why): a condition on the
    references that no host's float32 convolutions enter."""
    W, lms, ctx, emb_in, t64, t32 = L.reference(H.HEAD_FAULT_KIND, H.HEAD_FAULT_RECIPE)
    x32 = t64.acts[24].reshape(L.TOTAL, H.KDENSE).to(torch.float32)
    b64 = torch.from_numpy(W["last_dense/b"]).double().reshape(-1)
    iso64 = x32.double() @ torch.from_numpy(W["last_dense/w"]).double() + b64
    iso32 = H.dense_logits32_in_order(x32, W)
    assert torch.equal(iso32, H.dense_logits32_in_order(x32.clone(), W))
    for fault, (name, sl, bin_) in H.HEAD_FAULTS.items():
        g = H.head_fault_cpu_figures(fault)
        assert g["err_cpu32"] == float((iso32.double() - iso64).abs().max()) and g["m"] == float(iso64.abs().max())
        bar = max(K * g["err_cpu32"] + F * g["m"] for K, F in L.BAR.values())
        print("%s: slice %s: logits move by %.3e (%.2e of max); check_head bar %.3e (%.2e of max), 5 x %.3e; old bar %.1e" % (
            fault, sl, g["moved"], g["moved"] / g["m"], bar, bar / g["m"], 5 * bar, g["old_bar"]))
        assert g["changed"] == [name] == ["last_dense/w"], g["changed"]           # nothing before tensor 24 can move
        assert g["err_cpu32"] <= L.CAP * g["m"] and bar < L.CAP * g["m"]
        assert g["moved"] < g["old_bar"], (fault, g["moved"], g["old_bar"])
        assert g["moved"] >= 5 * bar, (fault, g["moved"], 5 * bar)
        moved = torch.nonzero(g["moved_by_bin"] > 0).flatten().tolist()
        assert (moved == [bin_]) if bin_ is not None else (len(moved) > 1 and max(moved) < 153), (fault, moved[:8])
        # ... and the comparison catches it with the float64 result of the planted weights in the device's place
        planted = x32.double() @ torch.from_numpy(H.plant_head(W, fault)[name]).double() + b64
        for mode in L.BAR:
            v = L.check_head("logits", planted.to(torch.float32), iso64, iso32, mode, "planted " + fault)
            assert not v.ok and "above the bar" in v.message
            must = set(torch.nonzero(g["moved_by_bin"] > 2 * v.bar).flatten().tolist())
            assert must and must <= set(v.channels_over), (fault, mode, sorted(must - set(v.channels_over)))
            if bin_ is not None:
                assert v.channels_over == [bin_] and v.worst[1] == bin_ and "bin %d)" % bin_ in v.message, v.message
                assert "1 of 201 bins above the bar: bin %d;" % bin_ in v.message, v.message
            else:
                assert len(v.channels_over) > 1


def test_pool_faults_are_caught_and_name_a_channel():
    """avgpool_kernel has no weights to plant a fault in: a mean that drops the last pixel (597, the one a loop bound one
    short loses) and a mean of the tensor rounded to f16 (the `lo` halves lost) in the device's place."""
    W, lms, ctx, emb_in, t64, t32 = L.reference(L.FAULT_KIND, L.FAULT_RECIPE)
    x7 = t32.acts[7]
    p = H.pool_refs(x7)
    x = x7.reshape(x7.shape[0], -1, H.EMB).double()
    assert x.shape[1] == H.POOL_PIXELS == 598
    dropped = x[:, :597].sum(dim=1) / 598.0
    halved = torch.from_numpy(L.r16(x7.numpy())).reshape(x7.shape[0], -1, H.EMB).double().mean(dim=1)
    for what, dev in (("pixel 597 dropped", dropped), ("tensor 7 rounded to f16", halved)):
        for mode in L.BAR:
            v = L.check_head("embeddings", dev.to(torch.float32), p["f64"], p["cpu32"], mode, what)
            print(what, v.row())
            assert not v.ok and v.err_hip > v.bar, (what, mode, v.row())
            r, c = v.worst
            assert "worst element (image %d, channel %d)" % (r, c) in v.message and v.channels_over, v.message
            assert "channel %d" % v.channels_over[0] in v.message
    # a good mean passes: the kernel's own order in float32
    for mode in L.BAR:
        assert L.check_head("embeddings", p["cpu32_kernel_order"], p["f64"], p["cpu32"], mode).ok


def test_check_head_says_where():
    """Rows are named by clip and position: the layer batch's frame 11 is the one-frame clip, frame 20 the last row."""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(L.TOTAL, H.BINS, generator=g, dtype=torch.float64)
    c32 = ref.to(torch.float32)
    for r, c, words in ((11, 200, ("clip 1", "first frame of clip 1", "last frame of clip 1")),
                        (20, 0, ("clip 2", "last frame of clip 2", "last row of a pass")),
                        (7, 64, ("clip 0", "last row of a pass"))):
        dev = c32.clone()
        dev[r, c] += 1e-3
        v = L.check_head("logits", dev, ref, c32, "f32", "moved one element", chunk=L.CHUNK)
        assert not v.ok and v.worst == (r, c) and v.channels_over == [c]
        assert "(frame %d, bin %d)" % (r, c) in v.message and all(w in v.message for w in words), v.message
    ok = L.check_head("denoised", c32, ref, c32, "f16x3")
    assert ok.ok and ok.message == "" and ok.row().startswith("27 head denoised")
    bad = c32.clone()
    bad[0, 0] = float("nan")
    assert not L.check_head("logits", bad, ref, c32, "f32").ok
    emb = torch.rand(3, H.EMB, generator=g, dtype=torch.float64)
    e32 = emb.to(torch.float32)
    dev = e32.clone()
    dev[2, 511] -= 1e-3
    v = L.check_head("embeddings", dev, emb, e32, "f32", chunk=2)
    assert not v.ok and "(image 2, channel 511)" in v.message and "last image" in v.message and v.channels_over == [511]


def test_canary_helper_reports_a_stray_store():
    for T in (1, 9):
        buf = H.guarded(T)
        assert buf.numel() == 2 * H.GUARD + T * H.BINS
        assert len(H.canary_damage(buf, T)) == 1 and "never written" in H.canary_damage(buf, T)[0]
        H.payload(buf, T)[:] = 1.5
        assert H.canary_damage(buf, T) == []
        # one word behind the last row -- where column 201 of the last row would land -- and one before row 0
        for word, where in ((H.GUARD + T * H.BINS, "after row %d" % (T - 1)), (H.GUARD - 1, "before row 0"),
                            (2 * H.GUARD + T * H.BINS - 1, "after row %d" % (T - 1))):
            hit = buf.clone()
            hit[word] = 0
            damage = H.canary_damage(hit, T)
            assert len(damage) == 1 and where in damage[0] and "1 sentinel words" in damage[0], damage
        # an output word left alone shows as well
        hole = buf.clone()
        hole[H.GUARD + T * H.BINS - 1] = H.SENTINEL
        assert "(row %d, bin 200)" % (T - 1) in H.canary_damage(hole, T)[0]
