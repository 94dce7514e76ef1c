"""Every element of every stored tensor of the HIP path against float64.

The library stores 25 tensors between its kernels (NHANS_NUM_ACTIVATIONS: 8 of the embedding tower, 16 of the residual
stack, last_conv).  nhans_debug_activation / nhans_debug_tower_activation copy any of them out of the PRODUCTION launches
(same plan, layouts, chunking, kernel variant, Winograd and split-K choices); here each is compared, all elements, with
oracle/torch_ref.py in float64 on identical float32 features and embeddings, for both models, three weight sets, both
arithmetic modes, the Winograd form on and off and (on one weight set) every conv variant and both tensor storages --
on a ragged batch of 11 + 1 + 9 frames whose launches end in partial tiles and whose tiles straddle frames and clips
(tests/layer_checks.py), and 3 context images of which one is the constant ln 1e-5.

Bar per tensor: K x max|cpu32 - f64| + F x max|f64| (the float32 CPU restatement is the yardstick, never the device),
capped below 2e-5 x max|f64|.  (K, F) per mode, layer_checks.BAR, from the measurement in profiles/layers/README.md;
its worst rows (MI355X, max|hip - f64| as a multiple of max|cpu32 - f64| and as a share of max|f64|):

    tensor  6 tower noise_resblock4_1 conv1   trained_bn  f32     5.95 x   3.60e-06      (bar 4 x + 2.4e-6: 6.57e-5 against 4.90e-5)
    tensor  7 tower noise_resblock4_1 output  synthetic7  f32     5.26 x   4.50e-06
    tensor  7 tower noise_resblock4_1 output  synthetic7  f16x3   5.01 x   4.29e-06      (every variant, Winograd on and off)
    tensor 23 stack resblock4_2 output        heavy       f32     5.00 x   3.36e-06
    tensor 20 stack resblock4_1 conv1         trained_bn  f32     4.10 x   3.25e-06
  650 tensor comparisons in all; float32 CPU against float64: 2.9e-7 .. 2.0e-6 of max; the largest bar 1.03e-5 of max.

Besides the bar: no negative value in a post-ReLU tensor, dead channels of `trained_bn` constant over pixels, and bit for
bit: one launch of all frames == passes of 8 frames, nhans_debug_block_output == the new tap, the tower for
contexts_per_chunk 64 / 1 / 2 and split_k 1 / 0; take_status() == 0 after every fetch; embeddings and logits of the same
engine at the existing bars -- and, element by element at the bar of the stored tensors, the three arrays a caller
receives: nhans_embed's embeddings, nhans_mask_net's logits and denoised rows (layer_checks.check_head; the code
between tensor 7 / 24 and them is tested alone in tests/test_gpu_heads.py).

test_planted_fault_is_caught_at_its_layer: the sensitivity of this file is itself under test.  A slice of one weight
tensor handed to the LIBRARY is rounded to f16 (for the arithmetic: a kernel that lost the `lo` half of that slice; no
kernel is touched), the reference keeps the true weights: the layer comparison must fail at exactly that tensor and name
the channel(s), while the logits / embeddings stay inside the bars the suite had before.
"""
import time

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine, hip
import layer_checks as L

pytestmark = pytest.mark.gpu

DEFAULTS = {"winograd": 1, "conv_variant": -1, "winograd_f32_tensors": 1, "frames_per_chunk": 3776,
            "contexts_per_chunk": 64, "split_k": 1}
CONFIGS = [("f32", "f32", {}), ("f16x3 winograd 1", "f16x3", {"winograd": 1}), ("f16x3 winograd 0", "f16x3", {"winograd": 0})]
# on one weight set: every conv variant of the split-f16 mode, and every tensor in split storage
EXTRA = [("f16x3 conv_variant %d" % v, "f16x3", {"conv_variant": v}) for v in (0, 1, 2)] + [
    ("f16x3 winograd_f32_tensors 0", "f16x3", {"winograd_f32_tensors": 0})]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _configure(eng, mode, options):
    eng.set_precision(mode)
    for k, v in DEFAULTS.items():
        eng.set_option(k, options.get(k, v))


class _Device:
    """One engine with the batch in HBM."""

    def __init__(self, kind, W, lms, ctx, emb_in):
        self.eng = engine.Engine(kind, W, precision="f16x3")
        self.lm = torch.from_numpy(np.concatenate(lms)).cuda()
        self.ctx = torch.from_numpy(ctx).cuda()
        ea, eb = L.clip_embeddings(np.asarray(emb_in, dtype=np.float32))
        self.ea, self.eb = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()

    def stack(self, idx, frames_per_chunk):
        self.eng.set_option("frames_per_chunk", frames_per_chunk)
        t = self.eng.activation(idx, self.lm, L.FOFF, self.ea, self.eb, 0, L.TOTAL)
        return t, self.eng.take_status()

    def block(self, idx):
        t = self.eng.block_output(self.lm, L.FOFF, self.ea, self.eb, 0, L.TOTAL, 8 if idx == 24 else (idx - 9) // 2)
        return t, self.eng.take_status()

    def tower(self, idx, contexts_per_chunk=64, split_k=1):
        self.eng.set_option("contexts_per_chunk", contexts_per_chunk)
        self.eng.set_option("split_k", split_k)
        t = self.eng.tower_activation(idx, self.ctx)
        return t, self.eng.take_status()

    def logits(self, frames_per_chunk=3776):
        self.eng.set_option("frames_per_chunk", frames_per_chunk)
        lg, _ = self.eng.mask_net(self.lm, L.FOFF, self.ea, self.eb)
        return lg, self.eng.take_status()

    def emb(self):
        e = self.eng.embed(self.ctx)
        return e, self.eng.take_status()

    def heads(self, frames_per_chunk=3776):
        """(logits, denoised) of one nhans_mask_net call."""
        self.eng.set_option("frames_per_chunk", frames_per_chunk)
        lg, den = self.eng.mask_net(self.lm, L.FOFF, self.ea, self.eb)
        return lg, den, self.eng.take_status()


def _averaged_bars(t64):
    return (L.LOGIT_TOL * max(1.0, float(t64.logits.abs().max()) / 5.0), L.EMB_TOL * max(1.0, float(t64.emb.abs().max())))


@pytest.mark.parametrize("recipe", list(L.WEIGHTS))
@pytest.mark.parametrize("kind", ["denoiser", "separator"])
def test_every_stored_tensor(lib_built, kind, recipe):
    L.check_batch_geometry()
    t0 = time.time()
    W, lms, ctx, emb_in, t64, t32 = L.reference(kind, recipe)
    t_ref = time.time() - t0
    logit_tol, emb_tol = _averaged_bars(t64)
    dev = _Device(kind, W, lms, ctx, emb_in)
    failures, rows = [], []
    try:
        for label, mode, options in CONFIGS + (EXTRA if recipe == "synthetic7" else []):
            _configure(dev.eng, mode, options)
            tag = "%s %s, %s" % (kind, recipe, label)

            def judge(idx, t, st, what):
                if st:
                    failures.append("%s: tensor %d %s left status %d" % (tag, idx, what, st))
                v = L.check_tensor(idx, t, t64, t32, mode, tag)
                rows.append("%-40s %s" % (tag, v.row()))
                if not v.ok:
                    failures.append(v.message)
                if recipe == "trained_bn":
                    dead, _ = L.dead_channels(W, idx)
                    if len(dead):
                        sub = t[..., torch.from_numpy(dead).to(t.device)]
                        spread = float((sub.amax(dim=(0, 1, 2)) - sub.amin(dim=(0, 1, 2))).max())
                        if spread != 0.0:
                            failures.append("%s: tensor %d (%s): a dead channel (gamma = 0) varies over pixels by %.3e" % (tag, idx, L.NAMES[idx], spread))

            # ---- stack + head: (a) all frames in one launch, (b) passes of 8 frames, the older block tap
            for idx in L.STACK_IDX:
                a, st = dev.stack(idx, DEFAULTS["frames_per_chunk"])
                b, st_b = dev.stack(idx, L.CHUNK)
                if st_b or not _same_bits(a, b):
                    failures.append("%s: tensor %d (%s): one launch and passes of %d frames differ (max %.3e, status %d)" % (
                        tag, idx, L.NAMES[idx], L.CHUNK, float((a - b).abs().max()), st_b))
                if idx % 2 or idx == 24:
                    o, st_o = dev.block(idx)
                    if st_o or not _same_bits(a, o):
                        failures.append("%s: tensor %d (%s): nhans_debug_block_output differs from the tap (max %.3e, status %d)" % (
                            tag, idx, L.NAMES[idx], float((a - o).abs().max()), st_o))
                judge(idx, a, st, "fetch")
            # ---- tower: 3 images; contexts_per_chunk and split-K leave the bits alone
            for idx in L.TOWER_IDX:
                a, st = dev.tower(idx)
                for cpc, sk in ((1, 1), (2, 1), (64, 0), (2, 0)):
                    b, st_b = dev.tower(idx, cpc, sk)
                    if st_b or not _same_bits(a, b):
                        failures.append("%s: tensor %d (%s): contexts_per_chunk %d split_k %d differs from 64 / 1 (max %.3e, status %d)" % (
                            tag, idx, L.NAMES[idx], cpc, sk, float((a - b).abs().max()), st_b))
                dev.eng.set_option("contexts_per_chunk", 64)
                dev.eng.set_option("split_k", 1)
                judge(idx, a, st, "fetch")
            # ---- the averaged outputs of the same engine at the bars the suite had before
            e, st_e = dev.emb()
            lg, st_l = dev.logits()
            lg_b, _ = dev.logits(L.CHUNK)
            e_err = float((e.cpu().double() - t64.emb).abs().max())
            l_err = float((lg.cpu().double() - t64.logits).abs().max())
            rows.append("%-40s embeddings err %.3e (bar %.1e)  logits err %.3e (bar %.1e)" % (tag, e_err, emb_tol, l_err, logit_tol))
            if st_e or st_l or not e_err < emb_tol or not l_err < logit_tol or not _same_bits(lg, lg_b):
                failures.append("%s: averaged outputs: embeddings %.3e (bar %.1e), logits %.3e (bar %.1e), status %d / %d, chunked logits same bits: %s" % (
                    tag, e_err, emb_tol, l_err, logit_tol, st_e, st_l, _same_bits(lg, lg_b)))
            # ---- the same three arrays, every element, at the bar of the stored tensors (layer_checks.check_head): one
            # launch of the ragged batch, which passes of 8 frames must repeat bit for bit -- the denoised rows too
            lg_h, den_h, st_h = dev.heads()
            lg_c, den_c, st_c = dev.heads(L.CHUNK)
            if st_h or st_c or not (_same_bits(lg_h, lg) and _same_bits(lg_c, lg_h) and _same_bits(den_c, den_h)):
                failures.append("%s: heads: one launch and passes of %d frames differ (logits %s, denoised %s, status %d / %d)" % (
                    tag, L.CHUNK, _same_bits(lg_c, lg_h) and _same_bits(lg_h, lg), _same_bits(den_c, den_h), st_h, st_c))
            for name, t, r64, r32 in (("embeddings", e, t64.emb, t32.emb), ("logits", lg_h, t64.logits, t32.logits),
                                      ("denoised", den_h, t64.denoised, t32.denoised)):
                v = L.check_head(name, t, r64, r32, mode, tag)
                rows.append("%-40s %s" % (tag, v.row()))
                if not v.ok:
                    failures.append(v.message)
    finally:
        dev.eng.close()
    print("\n%s %s: CPU references %.1f s, whole case %.1f s" % (kind, recipe, t_ref, time.time() - t0))
    print("\n".join(rows))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))


@pytest.mark.parametrize("fault", list(L.FAULTS))
def test_planted_fault_is_caught_at_its_layer(lib_built, fault):
    W, lms, ctx, emb_in, t64, t32 = L.reference(L.FAULT_KIND, L.FAULT_RECIPE)
    name, sl, target, chan = L.FAULTS[fault]
    g = L.fault_cpu_figures(fault)
    logit_tol, emb_tol = _averaged_bars(t64)
    old_bar = L.EMB_TOL if target < 8 else logit_tol            # (the embeddings' bar without its magnitude factor: the stricter reading)
    dev = _Device(L.FAULT_KIND, L.plant(W, fault), lms, ctx, emb_in)
    lines = []
    try:
        for mode in ("f32", "f16x3"):
            _configure(dev.eng, mode, {})
            K, F = L.BAR[mode]
            bar = K * g["err_cpu32"] + F * g["m"]
            # a valid witness (the CPU half, tests/test_oracle.py, asserts the same): blind at the old bar, 5 x the new one
            assert g["before"] == 0.0 and g["averaged"] < old_bar and g["own"] >= 5 * bar, (fault, mode, g, bar)
            verdicts = []
            for idx in ([i for i in L.TOWER_IDX if i <= target] if target < 8 else [i for i in L.STACK_IDX if i <= target]):
                t, st = dev.tower(idx) if idx < 8 else dev.stack(idx, DEFAULTS["frames_per_chunk"])
                assert st == 0
                verdicts.append(L.check_tensor(idx, t, t64, t32, mode, "planted " + fault))
            for v in verdicts[:-1]:
                assert v.ok, "a tensor BEFORE the planted fault fails: " + v.message
            v = verdicts[-1]
            assert not v.ok and v.err_hip > v.bar, (fault, mode, v.row())
            # where: every channel the fault moves by more than twice the bar in float64 must be named ...
            must = set(torch.nonzero(g["own_by_channel"] > 2 * bar).flatten().tolist())
            assert must and must <= set(v.channels_over), (fault, mode, sorted(must - set(v.channels_over)))
            # ... and for a fault in one output channel, that channel alone
            if chan is not None:
                assert v.channels_over == [chan] and v.worst[3] == chan, (fault, mode, v.channels_over, v.worst)
                assert "c %d)" % chan in v.message and "1 of " in v.message, v.message
            else:
                assert len(v.channels_over) > 1, (fault, mode, v.channels_over)
            # the averaged output of the same faulty engine passes the bar the suite had before
            if target < 8:
                out, st = dev.emb()
                avg = float((out.cpu().double() - t64.emb).abs().max())
            else:
                out, st = dev.logits()
                avg = float((out.cpu().double() - t64.logits).abs().max())
            assert st == 0 and avg < old_bar, (fault, mode, avg, old_bar)
            lines.append("%s %s: tensor %d: float64 CPU moves it by %.2e of max (device: %.2e of max, bar %.2e of max, %d channels "
                         "named); %s: float64 CPU %.2e, device against the true reference %.2e, old bar %.1e: blind" % (
                             fault, mode, target, g["own"] / g["m"], v.err_hip / v.m, v.bar / v.m, len(v.channels_over),
                             "embeddings" if target < 8 else "logits", g["averaged"], avg, old_bar))
    finally:
        dev.eng.close()
    print("\n" + "\n".join(lines))
