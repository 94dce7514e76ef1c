"""The context's workspace across calls of different sizes, through the C ABI: a call places its buffers against the
workspace as its own reserve left it -- reused, or freed and allocated anew -- and the offline path lets the tower's buffers
and the stack's share their place.

The contexts come from nhans_create_ex WITH activation exponents (read once from the module's ordinary engine): such a
context runs no calibration pass, so its workspace is empty until the first call.  On one of them, in order:

    1  nhans_score_rows      1 clip of 3 rows
    2  nhans_mask_net        1 clip of 5 frames, frames_per_chunk 2: three chunks, the workspace grows
    3  step 1 again          the workspace is reused, nothing grows
    4  nhans_enhance_clips   2 clips of 7 frames, contexts of 32,240 samples, contexts_per_chunk 1, frames_per_chunk 4: the
                             workspace grows again, tower and stack overlap
    5  step 2 again

Step 3 has the bits of step 1 and step 5 those of step 2; steps 2 and 4 each have the bits of the same call made as the FIRST
call of a fresh context with the same exponents and options; nhans_take_status is 0 throughout.  Precision f16x3."""
import ctypes

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import fold, hip, spec

pytestmark = pytest.mark.gpu

MASK_OPTIONS = {"frames_per_chunk": 2}
ENHANCE_OPTIONS = {"contexts_per_chunk": 1, "frames_per_chunk": 4}


class _HipError(AssertionError):
    pass


class _Ctx:
    """A context of nhans_create_ex with exponents, at f16x3; every call is followed by nhans_take_status == 0."""

    def __init__(self, world):
        self.w, self.lib, self.handle = world, hip.load(), ctypes.c_void_p()
        exps = (ctypes.c_int * hip.NUM_ACTIVATIONS)(*world["exps"])
        blob = world["blob"]
        self.ok(self.lib.nhans_create_ex(hip.DENOISER, blob.ctypes.data_as(ctypes.c_void_p), blob.size, world["eng"].device.index, exps,
                                         hip.NUM_ACTIVATIONS, ctypes.byref(self.handle)), "nhans_create_ex")
        self.options({"precision": 1})

    def ok(self, rc, what):
        if rc == -2:        # NHANS_EHIP: nothing more is started on the device
            raise _HipError("%s: %s" % (what, self.lib.nhans_last_error()))
        assert rc == 0, "%s: %s" % (what, self.lib.nhans_last_error())

    def options(self, opts):
        for k, v in opts.items():
            self.ok(self.lib.nhans_set_option(self.handle, k.encode(), v), "option " + k)

    def call(self, what, fn, *args):
        self.ok(fn(self.handle, *args, self.w["eng"]._stream()), what)
        flags = ctypes.c_int(-1)
        self.ok(self.lib.nhans_take_status(self.handle, ctypes.byref(flags), self.w["eng"]._stream()), what + ": nhans_take_status")
        assert flags.value == 0, "%s: status %d" % (what, flags.value)

    def close(self):
        if self.handle:
            self.lib.nhans_destroy(self.handle)
            self.handle = None

    # ---- the three calls: -> the bits of every output ----
    def score_rows(self):
        import torch
        w = self.w
        rec = torch.zeros(hip.SCORE_ROW_FIELDS, dtype=torch.float64, device=w["eng"].device)
        frames = torch.zeros(3 * 3, dtype=torch.float64, device=w["eng"].device)
        self.call("nhans_score_rows", self.lib.nhans_score_rows, hip.ptr(w["est"]), hip.ptr(w["tgt"]), hip.i64_array([0, 3]), 1,
                  hip.ptr(rec), hip.ptr(frames))
        return _bits(rec, frames)

    def mask_net(self):
        import torch
        w = self.w
        self.options(MASK_OPTIONS)
        lg, den = torch.zeros_like(w["lm"]), torch.zeros_like(w["lm"])
        self.call("nhans_mask_net", self.lib.nhans_mask_net, hip.ptr(w["lm"]), hip.i64_array([0, 5]), 1, hip.ptr(w["ea"]), hip.ptr(w["eb"]),
                  hip.ptr(lg), hip.ptr(den))
        return _bits(lg, den)

    def enhance_clips(self):
        import torch
        w = self.w
        self.options(ENHANCE_OPTIONS)
        d = w["eng"].device
        n, rows = w["mix"].numel(), (14, spec.BINS)
        den, mixed = torch.zeros(n, device=d), torch.zeros(n, device=d)
        lm, ph, lg = torch.zeros(rows, device=d), torch.zeros(rows, device=d), torch.zeros(rows, device=d)
        emb = torch.zeros(4 * spec.EMB, device=d)
        coff = hip.i64_array([0, hip.CAPTURE_SAMPLES, 2 * hip.CAPTURE_SAMPLES])
        self.call("nhans_enhance_clips", self.lib.nhans_enhance_clips, hip.ptr(w["mix"]), hip.i64_array([0, n // 2, n]), 2, hip.ptr(w["ca"]),
                  coff, hip.ptr(w["cb"]), coff, hip.ptr(den), hip.ptr(mixed), hip.ptr(lm), hip.ptr(ph), hip.ptr(lg), hip.ptr(emb))
        return _bits(den, mixed, lm, ph, lg, emb)


def _bits(*tensors):
    return [t.cpu().numpy().reshape(-1).view(np.uint32 if t.element_size() == 4 else np.uint64) for t in tensors]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def runs(lib_built, weights_denoiser):
    """Every call of the module, made once: the five steps on one context, then steps 2 and 4 first on a fresh one each."""
    import torch
    from nhans_amd import engine
    eng = engine.Engine("denoiser", weights_denoiser, precision="f16x3")
    made = []
    try:
        rng = np.random.default_rng(41)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)   # noqa: E731
        assert hip.CAPTURE_SAMPLES == 32240
        mix = dev(0.3 * rng.standard_normal(2 * (400 + 6 * 160)))
        ca, cb = (dev(0.2 * rng.standard_normal(2 * hip.CAPTURE_SAMPLES)) for _ in range(2))
        # the stage inputs of step 2 from the ordinary engine: 5 rows of clip 0, the embeddings of its two contexts
        lm, _ = eng.stft_features(mix[:400 + 4 * 160], [0, 400 + 4 * 160])
        ctx_lm, _ = eng.stft_features(torch.cat([ca[:hip.CAPTURE_SAMPLES], cb[:hip.CAPTURE_SAMPLES]]),
                                      [0, hip.CAPTURE_SAMPLES, 2 * hip.CAPTURE_SAMPLES], max_frames=spec.NOISE_WIN, want_phase=False)
        emb = eng.embed(ctx_lm.reshape(2, spec.NOISE_WIN, spec.BINS))
        tgt = rng.uniform(-12.0, 3.0, size=(3, spec.BINS))
        world = {"eng": eng, "exps": eng.activation_exponents(), "blob": np.frombuffer(fold.fold_weights(weights_denoiser, "denoiser"), dtype=np.uint8),
                 "mix": mix, "ca": ca, "cb": cb, "lm": lm.contiguous(), "ea": emb[0].contiguous(), "eb": emb[1].contiguous(),
                 "tgt": dev(tgt), "est": dev(tgt + 0.1 * rng.standard_normal(tgt.shape))}
        assert lm.shape == (5, spec.BINS) and eng.take_status() == 0
        out = {}
        one = _Ctx(world); made.append(one)
        out[1] = one.score_rows()
        out[2] = one.mask_net()
        out[3] = one.score_rows()
        out[4] = one.enhance_clips()
        out[5] = one.mask_net()
        fresh = _Ctx(world); made.append(fresh)
        out["mask_net first"] = fresh.mask_net()
        fresh = _Ctx(world); made.append(fresh)
        out["enhance_clips first"] = fresh.enhance_clips()
        yield out
    finally:
        for c in made:
            c.close()
        eng.close()


def test_outputs_are_computed(runs):
    """(what the comparisons below compare is not the zeros the buffers started with)"""
    for k, outs in runs.items():
        for i, o in enumerate(outs):
            assert np.any(o != 0), "step %s output %d is all zero" % (k, i)


def test_reused_workspace_same_bits(runs):
    assert _same(runs[3], runs[1])


def test_same_bits_after_the_workspace_grew_and_was_overwritten(runs):
    assert _same(runs[5], runs[2])


def test_grown_workspace_same_bits_as_first_call_of_a_fresh_context(runs):
    assert _same(runs[2], runs["mask_net first"])
    assert _same(runs[4], runs["enhance_clips first"])
