"""The two heads of the HIP path taken alone, every element against float64 (tests/head_checks.py).

Between the last stored tensor and the arrays a caller receives lies code that no convolution layer shares:
avgpool_kernel (tensor 7 -> embeddings), the dense launch of mask_net_run (tensor 24 -> logits, + centre row -> denoised:
K = 13,312 in 32 groups / split-K, 201 real of 256 padded columns, a row stride of 201 floats so that neither rows nor
chunk base pointers are 16-byte aligned, the pre-residual tap, an f32 identity) and cond_kernel (embeddings -> the 3,840
conditioning columns).  Here the device's own tap of tensor 24 / 7 is the INPUT, so the CPU does one float64 matrix
product or mean and the frame count is free: 1, 129, 257, 513 frames -- one below / above the conv kernels' 128-, 256- and
512-row tiles, a ragged last tile behind one, two and four full ones.

Bar: layer_checks.check_head -- K x max|cpu32 - f64| + F x max|f64| with the (K, F) and cap of the 25 stored tensors; the
yardstick is the same expression in torch float32 on the CPU, never the device.  The float32 restatement in the
kernel's documented order is recorded next to it.  profiles/heads/README.md holds the table of a run.

Besides the bar, bit for bit: split_k 1 == 0; frames_per_chunk 1 (9 frames) and 3 (10 frames) -- chunk base pointers
at every residue of g0 x 201 mod 4 -- == one launch; contexts_per_chunk 64 == 2 == 1; denoised == float32(centre) +
float32(logits), the order conv_epilogue.h states (aux is the pre-residual value, the residual is added by one fma with
idw = 1); 256 sentinel words before and after caller-owned logits / denoised buffers intact, every output word written.
One-hot embeddings pick single rows of cond.w.  Two faults planted in last_dense/w must fail at the logits, and only
there, with the bins named, while the averaged bar the suite had before passes.
"""
import ctypes

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine, hip
import head_checks as H
import layer_checks as L

pytestmark = pytest.mark.gpu

DEFAULTS = {"winograd": 1, "conv_variant": -1, "winograd_f32_tensors": 1, "frames_per_chunk": 3776,
            "contexts_per_chunk": 64, "split_k": 1}
MODES = ("f32", "f16x3")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _configure(eng, mode, options=None):
    eng.set_precision(mode)
    for k, v in DEFAULTS.items():
        eng.set_option(k, (options or {}).get(k, v))


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    e = engine.Engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


class _Exponents:
    """All activation exponents raised by `by` inside the block (f16x3: every stored tensor times 2^-by, the head's
    in_scale and the pool's `scale` other than the calibrated ones)."""

    def __init__(self, eng, by):
        self.eng, self.by = eng, by

    def __enter__(self):
        self.base = self.eng.activation_exponents()
        if self.by:
            self.eng.set_activation_exponents([e + self.by for e in self.base])
            assert self.eng.activation_exponents() != self.base

    def __exit__(self, *exc):
        self.eng.set_activation_exponents(self.base)


def _variants(mode, key):
    """(label, options, exponents raised by)"""
    if mode == "f32":
        return [("f32", {}, 0)]
    return [("f16x3", {}, 0), ("f16x3 %s 0" % key, {key: 0}, 0), ("f16x3 exponents +3", {}, 3)]


def _judge(rows, failures, name, got, refs, mode, tag, foff=None, chunk=0, which=None):
    """check_head at the torch float32 yardstick; the figures of the kernel-order float32 restatement beside it."""
    pick = (lambda r: r) if which is None else (lambda r: r[which])
    other = [k for k in refs if k not in ("f64", "cpu32")][0]
    v = L.check_head(name, got, pick(refs["f64"]), pick(refs["cpu32"]), mode, tag, foff=foff, chunk=chunk)
    alt = float((pick(refs[other]).double() - pick(refs["f64"])).abs().max())
    rows.append("%-44s %s   [%s err %.3e]" % (tag, v.row(), other, alt))
    if not v.ok:
        failures.append(v.message)
    return v


# ---- dense head -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", H.DENSE_T)
@pytest.mark.parametrize("mode", MODES)
def test_dense_head_alone(eng, weights_denoiser, mode, T):
    W = weights_denoiser
    rows, failures = [], []
    for foff in ([None] if T != 513 else [None, H.CLIPS_513]):
        lm, foff, ea, eb = H.dense_inputs(T, foff)
        lm_d, ea_d, eb_d = lm.cuda(), ea.cuda(), eb.cuda()
        first = None
        for label, options, raised in _variants(mode, "split_k"):
            tag = "dense T %d, %d clip%s, %s" % (T, len(foff) - 1, "" if len(foff) == 2 else "s", label)
            _configure(eng, mode, options)
            try:
                with _Exponents(eng, raised):
                    x24 = eng.activation(24, lm_d, foff, ea_d, eb_d, 0, T)
                    st_x = eng.take_status()
                    lg, den = eng.mask_net(lm_d, foff, ea_d, eb_d)
                    st = eng.take_status()
            finally:
                _configure(eng, mode)
            if st_x or st:
                failures.append("%s: status %d / %d" % (tag, st_x, st))
            refs = H.dense_refs(x24, W, lm)
            _judge(rows, failures, "logits", lg, refs, mode, tag, foff, which=0)
            _judge(rows, failures, "denoised", den, refs, mode, tag, foff, which=1)
            # the identity term: aux is the pre-residual value, out = fma(1, centre, aux) -- one rounding of the sum
            if not _same_bits(den, lm_d + lg):
                failures.append("%s: denoised != float32(centre) + float32(logits) (max %.3e)" % (tag, float((den - (lm_d + lg)).abs().max())))
            # split_k 1 (the first variant) and split_k 0 (the second) at the calibrated exponents: the same bits
            if not options and not raised:
                first = (lg, den)
            elif "split_k" in options and not (_same_bits(lg, first[0]) and _same_bits(den, first[1])):
                    failures.append("%s: split_k 0 and 1 differ (logits max %.3e)" % (tag, float((lg - first[0]).abs().max())))
    print("\n" + "\n".join(rows))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))


@pytest.mark.parametrize("T,fpc", [(9, 1), (10, 3)])
@pytest.mark.parametrize("mode", MODES)
def test_dense_head_chunk_pointers_at_every_alignment(eng, mode, T, fpc):
    """Chunk g0's outputs start at denoised + g0 x 201 floats: g0 x 201 mod 4 = g0 mod 4 for passes of 1 frame (all four
    residues in 9 frames), and passes of 3 frames start at g0 = 0, 3, 6, 9: residues 0, 3, 2, 1."""
    assert {(g0 * H.BINS) % 4 for g0 in range(0, T, fpc)} == {0, 1, 2, 3}
    lm, foff, ea, eb = H.dense_inputs(T)
    lm_d, ea_d, eb_d = lm.cuda(), ea.cuda(), eb.cuda()
    _configure(eng, mode)
    try:
        lg, den = eng.mask_net(lm_d, foff, ea_d, eb_d)
        st = eng.take_status()
        eng.set_option("frames_per_chunk", fpc)
        lg_c, den_c = eng.mask_net(lm_d, foff, ea_d, eb_d)
        st_c = eng.take_status()
    finally:
        _configure(eng, mode)
    assert st == 0 and st_c == 0
    assert _same_bits(lg, lg_c), "logits: passes of %d differ from one launch by %.3e" % (fpc, float((lg - lg_c).abs().max()))
    assert _same_bits(den, den_c), "denoised: passes of %d differ from one launch by %.3e" % (fpc, float((den - den_c).abs().max()))
    assert _same_bits(den, lm_d + lg)


@pytest.mark.parametrize("T", [1, 9])
@pytest.mark.parametrize("mode", MODES)
def test_dense_head_leaves_the_words_around_its_outputs_alone(eng, mode, T):
    """nhans_mask_net itself with caller-owned buffers: the launch computes 256 columns for 201 real ones, and a stray
    store of columns 201..255 of the last row -- or of a row before the first, in a chunk at an odd base pointer -- lands
    in the 256 sentinel words after / before the outputs."""
    lib = hip.load()
    lm, foff, ea, eb = H.dense_inputs(T)
    lm_d, ea_d, eb_d = lm.cuda(), ea.cuda(), eb.cuda()
    _configure(eng, mode)
    try:
        want_lg, want_den = eng.mask_net(lm_d, foff, ea_d, eb_d)
        assert eng.take_status() == 0
        for fpc in (DEFAULTS["frames_per_chunk"], 1):
            eng.set_option("frames_per_chunk", fpc)
            lg_buf, den_buf = H.guarded(T, "cuda"), H.guarded(T, "cuda")
            torch.cuda.synchronize()
            hip.check(lib.nhans_mask_net(eng.handle, hip.ptr(lm_d), hip.i64_array(foff), 1, hip.ptr(ea_d), hip.ptr(eb_d),
                                         ctypes.c_void_p(lg_buf.data_ptr() + 4 * H.GUARD),
                                         ctypes.c_void_p(den_buf.data_ptr() + 4 * H.GUARD), eng._stream()))
            assert eng.take_status() == 0
            for what, buf, want in (("logits", lg_buf, want_lg), ("denoised", den_buf, want_den)):
                damage = H.canary_damage(buf, T)
                assert not damage, "%s, %d frames, frames_per_chunk %d, %s: %s" % (mode, T, fpc, what, "; ".join(damage))
                assert _same_bits(H.payload(buf, T), want), (mode, T, fpc, what)
    finally:
        _configure(eng, mode)


# ---- pool head --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cpc", [(1, 64), (5, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_pool_head_alone(eng, mode, n, cpc):
    """n = 5 in passes of 2 images: [0, 2), [2, 4), [4, 5) -- a non-zero first image and a short last pass; the last image
    is the constant ln 1e-5."""
    ctx = H.pool_contexts(n)
    ctx_d = ctx.cuda()
    rows, failures = [], []
    for label, options, raised in _variants(mode, "winograd_f32_tensors"):
        tag = "pool n %d, contexts_per_chunk %d, %s" % (n, cpc, label)
        _configure(eng, mode, dict(options, contexts_per_chunk=cpc))
        try:
            with _Exponents(eng, raised):
                x7 = eng.tower_activation(7, ctx_d)
                st_x = eng.take_status()
                e = eng.embed(ctx_d)
                st = eng.take_status()
                for other in (64, 2, 1):
                    eng.set_option("contexts_per_chunk", other)
                    e_o = eng.embed(ctx_d)
                    if eng.take_status() or not _same_bits(e, e_o):
                        failures.append("%s: contexts_per_chunk %d differs from %d by %.3e" % (tag, other, cpc, float((e - e_o).abs().max())))
        finally:
            _configure(eng, mode)
        if st_x or st:
            failures.append("%s: status %d / %d" % (tag, st_x, st))
        assert tuple(x7.shape) == (n, 23, 26, 512)
        _judge(rows, failures, "embeddings", e, H.pool_refs(x7), mode, tag, chunk=cpc)
    print("\n" + "\n".join(rows))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))


# ---- one-hot conditioning ---------------------------------------------------------------------------------------------
_onehot = {}


def _onehot_reference(W):
    if not _onehot:
        _onehot["t64"] = H.onehot_taps(W, "denoiser", torch.float64)
        _onehot["t32"] = H.onehot_taps(W, "denoiser", torch.float32)
    return _onehot["t64"], _onehot["t32"]


@pytest.mark.parametrize("mode", MODES)
def test_one_hot_embeddings_pick_single_rows_of_the_conditioning_weights(eng, weights_denoiser, mode):
    """Four one-frame clips conditioned on zeros / zeros, e0 / zeros, e511 / e256, zeros / e511: cond_kernel's 1,024 x 3,840
    product reduces to single rows of cond.w -- first and last of each half --, for clip indices up to 3; seen at the
    first and last block's tensors (the first and last column groups of the 3,840) and at the logits."""
    t64, t32 = _onehot_reference(weights_denoiser)
    ea, eb = H.onehot_embeddings()
    lm_d = torch.from_numpy(H.onehot_logmag()).cuda()
    ea_d, eb_d = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
    rows, failures = [], []
    _configure(eng, mode)
    try:
        for idx in H.ONEHOT_TENSORS:
            t = eng.activation(idx, lm_d, H.ONEHOT_FOFF, ea_d, eb_d, 0, 4)
            assert eng.take_status() == 0
            v = L.check_tensor(idx, t, t64, t32, mode, "one-hot embeddings, four one-frame clips")
            rows.append("%-44s %s" % ("one-hot " + mode, v.row()))
            if not v.ok:
                failures.append(v.message)
        lg, den = eng.mask_net(lm_d, H.ONEHOT_FOFF, ea_d, eb_d)
        assert eng.take_status() == 0
    finally:
        _configure(eng, mode)
    for name, got, r64, r32 in (("logits", lg, t64.logits, t32.logits), ("denoised", den, t64.denoised, t32.denoised)):
        v = L.check_head(name, got, r64, r32, mode, "one-hot embeddings", foff=H.ONEHOT_FOFF)
        rows.append("%-44s %s" % ("one-hot " + mode, v.row()))
        if not v.ok:
            failures.append(v.message)
    print("\n" + "\n".join(rows))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))


# ---- faults planted in last_dense/w -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", list(H.HEAD_FAULTS))
def test_planted_head_fault_is_caught_at_the_logits(lib_built, fault):
    """A slice of last_dense/w handed to the LIBRARY is rounded to f16, the reference keeps the true weights: check_head must
    fail on the logits and name the bins -- on the layer batch against the whole-stack references, and with the device's own
    tensor 24 as the input of the true float64 product --, tensor 24 of the same engine must pass check_tensor, and the
    averaged bar the suite had before must pass: blind.  (That each slice is a valid witness is a statement about the CPU
    references and is asserted in tests/test_head_checks_host.py.  The references here are `separator heavy`, not the set
    the layer tests cache last: this test pays one CPU reference of its own, some 10 s, shared by its two cases.)"""
    W, lms, ctx, emb_in, t64, t32 = L.reference(H.HEAD_FAULT_KIND, H.HEAD_FAULT_RECIPE)
    g = H.head_fault_cpu_figures(fault)
    assert g["changed"] == ["last_dense/w"] and g["moved"] < g["old_bar"], (fault, g)
    bin_ = H.HEAD_FAULTS[fault][2]
    lm = torch.from_numpy(np.concatenate(lms))
    lm_d = lm.cuda()
    ea, eb = L.clip_embeddings(np.asarray(emb_in, dtype=np.float32))
    ea_d, eb_d = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
    eng = engine.Engine(H.HEAD_FAULT_KIND, H.plant_head(W, fault), precision="f16x3")
    lines = []
    try:
        for mode in MODES:
            _configure(eng, mode)
            x24 = eng.activation(24, lm_d, L.FOFF, ea_d, eb_d, 0, L.TOTAL)
            assert eng.take_status() == 0
            v24 = L.check_tensor(24, x24, t64, t32, mode, "planted " + fault)
            assert v24.ok, "tensor 24, BEFORE the planted fault, fails: " + v24.message
            lg, den = eng.mask_net(lm_d, L.FOFF, ea_d, eb_d)
            assert eng.take_status() == 0
            refs = H.dense_refs(x24, W, lm)                      # the TRUE weights on the device's own tensor 24
            for what, v in (("whole stack", L.check_head("logits", lg, t64.logits, t32.logits, mode, "planted " + fault)),
                            ("head alone", L.check_head("logits", lg, refs["f64"][0], refs["cpu32"][0], mode, "planted " + fault))):
                lines.append("%-44s %s" % ("planted %s, %s" % (fault, what), v.row()))
                assert not v.ok and v.err_hip > v.bar, (fault, mode, what, v.row())
                # where: every bin the fault moves by more than twice the bar in float64 must be named ...
                must = set(torch.nonzero(g["moved_by_bin"] > 2 * v.bar).flatten().tolist())
                assert must <= set(v.channels_over), (fault, mode, what, sorted(must - set(v.channels_over)))
                # ... and for the fault in one bin, that bin alone
                if bin_ is not None:
                    assert v.channels_over == [bin_] and v.worst[1] == bin_, (fault, mode, what, v.channels_over, v.worst)
                    assert "bin %d)" % bin_ in v.message and "1 of 201 bins above the bar: bin %d;" % bin_ in v.message, v.message
                else:
                    assert len(v.channels_over) > 1 and max(v.channels_over) < 153, (fault, mode, what, v.channels_over)
            # the averaged output of the same faulty engine passes the bar the suite had before
            avg = float((lg.cpu().double() - t64.logits).abs().max())
            assert avg < g["old_bar"], (fault, mode, avg, g["old_bar"])
            lines.append("%s %s: float64 CPU moves the logits by %.2e of max; device against the true reference %.3e, old bar %.1e: "
                         "blind; tensor 24 passes (%.2e of max, bar %.2e)" % (
                             fault, mode, g["moved"] / g["m"], avg, g["old_bar"], v24.err_hip / v24.m, v24.bar / v24.m))
    finally:
        eng.close()
    print("\n" + "\n".join(lines))
