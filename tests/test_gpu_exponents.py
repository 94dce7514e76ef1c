"""Stored tensors across the exponent range: parity with float64 and the saturation flag, one tie group at a time.

In f16x3 mode every tensor between two kernels is hi + lo f16 at a per-tensor power-of-two exponent (the 25
NHANS_NUM_ACTIVATIONS, those that stored_f32() keeps in f32 included: scaled and clamped the same way).  The exponents
move in production -- the built-in calibration, cached exponents taken on trust, Engine.calibrate, the raise-only update
after a saturated batch -- and tests/test_gpu_layers.py holds the tensors to float64 only where the built-in calibration
put them, tests/test_gpu_scale.py moves all exponents at once and looks at the logits.  Here (tests/exponent_checks.py
has the helpers and the reasoning) every tie group in turn is moved alone, all others at the engine's own exponents, to

    tight    largest stored maximum of the group in [3500, 7000)     just inside the Winograd-input limit 7168
    between  [16000, 32000)                                          outside it, inside f16's 65504
    over     [2^17, 2^18)                                            clamped: the flag is this writer's alone
    raised   base + k (exponent_checks.K_RAISED)                     lo halves, then hi halves, are f16 subnormals

and the group's tensors, the next stored tensor (their reader) and the heads are fetched from the production launches
and held, all elements, to float64 at the UNCHANGED bar of the layer tests (a power of two towards larger stored values
is exact); what the status must be comes from the float64 maxima (exponent_checks.verdict_of), never from the device.
`over`: status 0 before the group's writer ran, STATUS_SATURATED after it, 0 on the second read; every element beyond
1.1 x 65504 is 65504 x 2^e exactly, every element below 0.9 x 65504 inside the bar.  `raised`: status 0 and
bar_j + 4 fmt_j, fmt_j what the storage format itself costs in float64 on the CPU (one pass per group, shared by the
configurations); tests/test_exponent_checks_host.py proves that a path flushing subnormal halves would fail there.

Configurations, one option off its default at a time: winograd, conv_variant, row_split, winograd_f32_tensors,
frames_per_chunk (stack), contexts_per_chunk and split_k (tower) on `synthetic7`; defaults and winograd 0 on `trained_bn`
and the separator.  profiles/exponents/README.md holds the measured tables.
"""
import time

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine, hip
import layer_checks as L
import exponent_checks as X

pytestmark = pytest.mark.gpu

DEFAULTS = {"winograd": 1, "conv_variant": -1, "row_split": 1, "winograd_f32_tensors": 1, "frames_per_chunk": 3776,
            "contexts_per_chunk": 64, "split_k": 1}
# (label, options, networks the option reaches)
CONFIGS = [("defaults", {}, "tower stack"), ("winograd 0", {"winograd": 0}, "tower stack")] + [
    ("conv_variant %d" % v, {"conv_variant": v}, "tower stack") for v in (0, 1, 2)] + [
    ("row_split 0", {"row_split": 0}, "stack"), ("winograd_f32_tensors 0", {"winograd_f32_tensors": 0}, "stack"),
    ("frames_per_chunk 8", {"frames_per_chunk": L.CHUNK}, "stack"),
    ("contexts_per_chunk 1", {"contexts_per_chunk": 1}, "tower"), ("split_k 0", {"split_k": 0}, "tower")]
# case-major, so that the cached reference, its copy on the device and the engine serve every configuration of a case
MATRIX = [(kind, recipe, c) for kind, recipe in X.CASES for c in (CONFIGS if recipe == "synthetic7" and kind == "denoiser" else CONFIGS[:2])]


class _Device:
    """One engine with the batch in HBM (the pattern of tests/test_gpu_layers.py) behind exponent_checks' interface."""

    def __init__(self, yard):
        self.eng = engine.Engine(yard.kind, yard.W, precision="f16x3")
        self.lm = torch.from_numpy(np.concatenate(yard.lms)).cuda()
        self.ctx = torch.from_numpy(yard.ctx).cuda()
        ea, eb = L.clip_embeddings(np.asarray(yard.emb_in, dtype=np.float32))
        self.ea, self.eb = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
        self.base = self.eng.activation_exponents()

    def set_exponents(self, E):
        self.eng.set_activation_exponents(E)
        return self.eng.activation_exponents()

    def take_status(self):
        return self.eng.take_status()

    def fetch(self, i):
        if i < 8:
            t = self.eng.tower_activation(i, self.ctx)
        elif i < 25:
            t = self.eng.activation(i, self.lm, L.FOFF, self.ea, self.eb, 0, L.TOTAL)
        elif i == X.EMB:
            t = self.eng.embed(self.ctx)
        else:
            t = self.eng.mask_net(self.lm, L.FOFF, self.ea, self.eb)
        return t, self.eng.take_status()

    def configure(self, options):
        self.eng.set_precision("f16x3")
        for k, v in DEFAULTS.items():
            self.eng.set_option(k, options.get(k, v))


_case = [None, None, None]


def _open(kind, recipe):
    """(yard on the device, engine) of one case; the last one asked for is kept."""
    if _case[0] != (kind, recipe):
        _close()
        yard = X.Yard(kind, recipe, device="cuda")
        _case[:] = [(kind, recipe), yard, _Device(yard)]
    return _case[1], _case[2]


def _close():
    if _case[2] is not None:
        _case[2].eng.close()
    _case[:] = [None, None, None]


@pytest.fixture(scope="module", autouse=True)
def _engines(lib_built):
    yield
    _close()


def _run(kind, recipe, label, options, nets, positions, sink=None):
    t0 = time.time()
    yard, dev = _open(kind, recipe)
    t_ref = time.time() - t0
    failures, rows = [], []
    tag = "%s %s, %s" % (kind, recipe, label)
    try:
        dev.configure(options)
        assert dev.take_status() == 0
        for g in X.groups():
            if ("tower" if g[0] < 8 else "stack") not in nets:
                continue
            for pos in positions:
                f, r = X.check_position(dev, yard, dev.base, g, pos, options.get("winograd", 1), tag,
                                        k=X.K_RAISED[(kind, recipe)] if pos == "raised" else None, sink=sink)
                failures += f
                rows += r
    finally:
        dev.configure({})
        dev.set_exponents(dev.base)
        dev.take_status()
    print("\n%s: engine exponents %s; reference and engine %.1f s, whole case %.1f s" % (tag, dev.base, t_ref, time.time() - t0))
    print("\n".join(rows))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures))


@pytest.mark.parametrize("kind,recipe,config", MATRIX, ids=["%s-%s-%s" % (k, r, c[0].replace(" ", "_")) for k, r, c in MATRIX])
def test_every_writer_clamps_with_the_flag_and_is_quiet_inside_the_limits(kind, recipe, config):
    label, options, nets = config
    _run(kind, recipe, label, options, nets, ("tight", "between", "over"))


@pytest.mark.parametrize("kind,recipe", X.CASES)
def test_raised_exponents_keep_the_subnormal_halves(kind, recipe):
    """Status 0, and tensor, reader and heads within bar + 4 x the format's own cost (exponent_checks.Yard.fmt), with the
    Winograd form on and off.  Measured on the MI355X (profiles/exponents/README.md): the worst (err - bar) / fmt of the
    run is printed below the rows."""
    for label, options in (("defaults", {}), ("winograd 0", {"winograd": 0})):
        sink = []
        try:
            _run(kind, recipe, label, options, "tower stack", ("raised",), sink=sink)
        finally:
            worst = max(sink, key=lambda s: (s["err"] - s["bar"]) / s["fmt"] if s["fmt"] else -1e30, default=None)
            if worst:
                print("%s %s, %s, k %d: worst (err - bar) / fmt %.2f at tensor %d (err/max %.2e, fmt/max %.2e)" % (
                    kind, recipe, label, X.K_RAISED[(kind, recipe)], (worst["err"] - worst["bar"]) / worst["fmt"], worst["tensor"],
                    worst["err"] / worst["m"], worst["fmt"] / worst["m"]))


def test_engine_exponents_are_the_ones_the_witness_was_checked_at(lib_built):
    """The device-free half proves the flush witness at exponent_checks.ENGINE_BASE: the built-in calibration must still
    put the engine there (it is deterministic), or that proof speaks of other exponents."""
    for kind, recipe in X.CASES:
        yard, dev = _open(kind, recipe)
        assert dev.base == X.ENGINE_BASE[(kind, recipe)], (kind, recipe, dev.base)
        assert hip.STATUS_SATURATED == X.SATURATED
