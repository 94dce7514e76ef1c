"""Calibration: the recorded maxima and the chosen exponents against float64.

In the split-f16 mode every stored tensor lives at a per-tensor power-of-two exponent, and the exponents come from a
calibration bracket (include/nhans_hip.h, option "calibrate"): absmax_kernel records the largest |x| at every tap() point
of the production launches, finish_calibration / tie_exponents turn the maxima into exponents.  The rest of the suite
pins everything downstream of the exponents; here the maxima (nhans_get_activation_amax) are held to the TRUE maxima of
the tensors -- the float64 reference of tests/layer_checks.py, at the layer tests' own bar, which bounds a maximum as it
bounds every element (tests/calibration_checks.py has the helpers and the reasoning) -- and the exponents to the header's
rule applied to the float64 maxima, which tests/test_calibration_checks_host.py proves unambiguous for every case here.

The batch is the layer tests': 11 + 1 + 9 frames, 3 context images.  Cases: exponent_checks.CASES and
`denoiser / one_channel_loud`, whose maxima sit in channels 0, 31, 32 and C - 1 in turn.  Brackets are opened round
mask_net, embed, activation and tower_activation:

  * maxima at precision 0: the whole batch in one launch; in passes of 8 frames / 1 image (same bits); per clip; per
    frame (21 brackets); per image; the maximum over frames and images is the whole batch's bit for bit
  * the tap and the maximum read one buffer: amax[j] has the bits of max|returned tensor j|
  * exponents: the rule applied to the float64 maxima, and -- exactly -- to the maxima as reported; tie pairs equal
  * raise only (close with 2), tensors a bracket does not write, a discarded bracket (3), zero maxima at the next open
  * a bracket at precision 1, status 0, three configurations: bar + 2^-11 max for the tensors read through hi halves
  * the built-in calibration of nhans_create is a user bracket at precision 0 round enhance_device of the batch
    nhans_debug_builtin_batch exports, bit for bit.

Every test prints its worst ratio to the bar; profiles/calibration/README.md keeps the tables.  The host half plants six
faults of a maximum kernel into an emulated device and shows each rejected by these very checks.
"""
import time

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine, hip
import layer_checks as L
import exponent_checks as X
import calibration_checks as C

pytestmark = pytest.mark.gpu

DEFAULTS = {"winograd": 1, "winograd_f32_tensors": 1, "frames_per_chunk": 3776, "contexts_per_chunk": 64}
CONFIGS_P1 = [("defaults", {}, C.F32_STORED), ("winograd_f32_tensors 0", {"winograd_f32_tensors": 0}, ()), ("winograd 0", {"winograd": 0}, ())]
IDS = ["%s-%s" % c for c in C.CASES]


class _Device:
    """One engine with the batch in HBM behind calibration_checks' interface."""

    def __init__(self, yard):
        self.eng = engine.Engine(yard.kind, yard.W, precision="f16x3")
        self.base = self.eng.activation_exponents()             # what the built-in calibration left
        self.amax0 = self.eng.activation_amax()
        self.lm = torch.from_numpy(np.concatenate(yard.lms)).cuda()
        self.ctx = torch.from_numpy(yard.ctx).cuda()
        ea, eb = L.clip_embeddings(np.asarray(yard.emb_in, dtype=np.float32))
        self.ea, self.eb = torch.from_numpy(ea).cuda(), torch.from_numpy(eb).cuda()
        self.last_outputs, self.last_status = [], 0

    def exponents(self):
        return self.eng.activation_exponents()

    def set_exponents(self, E):
        self.eng.set_activation_exponents(E)
        return self.eng.activation_exponents()

    def _run(self, call):
        what = call[0]
        if what == "mask_net":
            if call[1] is None:
                return self.eng.mask_net(self.lm, L.FOFF, self.ea, self.eb)
            i, lo, hi = call[1], L.FOFF[call[1]], L.FOFF[call[1] + 1]
            return self.eng.mask_net(self.lm[lo:hi].contiguous(), [0, hi - lo], self.ea[i:i + 1], self.eb[i:i + 1])
        if what == "embed":
            return self.eng.embed(self.ctx if call[1] is None else self.ctx[call[1]:call[1] + 1])
        if what == "activation":
            return self.eng.activation(call[1], self.lm, L.FOFF, self.ea, self.eb, call[2], call[3])
        if what == "tower_activation":
            return self.eng.tower_activation(call[1], self.ctx)
        raise KeyError(call)

    def bracket(self, calls, close, precision=0, options=None):
        options = options or {}
        try:
            self.eng.set_precision("f16x3" if precision else "f32")
            for k, v in DEFAULTS.items():
                self.eng.set_option(k, options.get(k, v))
            self.eng.set_option("calibrate", 1)
            try:
                self.last_outputs = [self._run(c) for c in calls]
            except BaseException:
                self.eng.set_option("calibrate", 3)
                raise
            self.eng.set_option("calibrate", close)
            self.last_status = self.eng.take_status()
        finally:
            self.eng.set_precision("f16x3")
            for k, v in DEFAULTS.items():
                self.eng.set_option(k, v)
        return self.eng.activation_amax(), self.eng.activation_exponents()


_case = [None, None, None, None]


def _open(kind, recipe):
    """(yard, float64 maxima, engine) of one case; the last one asked for is kept."""
    if _case[0] != (kind, recipe):
        _close()
        yard = X.Yard(kind, recipe)
        _case[:] = [(kind, recipe), yard, C.Maxima(yard), _Device(yard)]
    return _case[1], _case[2], _case[3]


def _close():
    if _case[3] is not None:
        _case[3].eng.close()
    _case[:] = [None, None, None, None]


@pytest.fixture(scope="module", autouse=True)
def _engines(lib_built):
    yield
    _close()


@pytest.fixture(scope="module", params=C.CASES, ids=IDS)
def case(request):
    return request.param


def _finish(rep, dev, t0):
    print("\n%s: engine exponents %s, %.1f s\n%s" % (rep.label, dev.base, time.time() - t0, rep.table()))
    assert dev.eng.take_status() == 0
    assert dev.exponents() == dev.base, "a check left the exponents moved"
    assert not rep.failures, "%d failures:\n%s" % (len(rep.failures), "\n".join(rep.failures))


def test_recorded_maxima_are_the_float64_maxima_at_every_scope(case):
    """Precision 0.  Whole batch, passes of 8 frames and 1 image (same bits), per clip, per frame, per image: every
    amax[j] within bar_j of the float64 maximum of what the bracket wrote, 0 for what it did not; after the whole-batch
    brackets the exponents are the rule applied to the float64 maxima; after every bracket, to the reported ones."""
    t0 = time.time()
    yard, mx, dev = _open(*case)
    rep = C.Report("%s %s" % case)
    C.check_scopes(dev, yard, mx, rep)
    _finish(rep, dev, t0)


def test_tap_and_maximum_read_the_same_buffer(case):
    """A bracket round activation(j) / tower_activation(j) at precision 0: amax[j] has exactly the bits of
    max|returned tensor|, and the tensors before it in the launch sequence are within the bar as well."""
    t0 = time.time()
    yard, mx, dev = _open(*case)
    rep = C.Report("%s %s" % case)
    try:
        for j in range(25):
            calls = [("tower_activation", j)] if j < 8 else [("activation", j, 0, L.TOTAL)]
            amax, _ = C.check_bracket(dev, yard, mx, calls, "tap [%d]" % j, rep)
            dev.set_exponents(dev.base)
            t = dev.last_outputs[0]
            m = float(t.abs().max())
            if not (float(np.float32(amax[j])) == m and m > 0 and dev.last_status == 0):
                rep.add("tap [%d]" % j, ["%s: tensor %d (%s): recorded maximum %.9g, max|tap| %.9g, status %d" % (
                    rep.label, j, L.NAMES[j], amax[j], m, dev.last_status)])
    finally:
        dev.set_exponents(dev.base)
    _finish(rep, dev, t0)


def test_raise_only_untouched_tensors_and_a_fresh_bracket(case):
    """Close with 2 from exponents -2 / +2 round the rule's: the rule merged with what was read back.  A bracket round
    embed alone, and one round activation(13), leave every other exponent where it was (3 above the rule's); a bracket
    closed with 3 moves none; the bracket after it -- the one-frame clip after the whole batch -- starts from zero."""
    t0 = time.time()
    yard, mx, dev = _open(*case)
    rep = C.Report("%s %s" % case)
    C.check_raise_only(dev, yard, mx, rep)
    C.check_untouched(dev, yard, mx, rep)
    _finish(rep, dev, t0)


def test_bracket_at_precision_1(case):
    """The header allows a bracket at any precision.  At the engine's own exponents, status 0: every amax[j] within
    bar_j + 2^-11 max_j of float64 -- the second term for the tensors read through their hi halves only; with the
    defaults tensors 8, 9, 10, 13 and 14 are f32 words (the f32_layout branch of tap()) and get none."""
    t0 = time.time()
    yard, mx, dev = _open(*case)
    rep = C.Report("%s %s" % case)
    for name, options, f32_stored in CONFIGS_P1:
        sub = C.Report("%s %s, %s" % (case + (name,)))
        C.check_precision_1(dev, yard, mx, sub, options=options, f32_stored=f32_stored)
        if dev.last_status:
            sub.failures.append("%s: status %d after the bracket at precision 1" % (sub.label, dev.last_status))
        rep.failures += sub.failures
        rep.worst.update({"%s, %s" % (k, name): v for k, v in sub.worst.items()})
    _finish(rep, dev, t0)


def test_builtin_calibration_is_a_user_bracket_on_the_exported_batch(case):
    """What nhans_create left on a fresh engine -- maxima and exponents -- is, bit for bit, what a bracket at precision 0
    round enhance_device of the batch of nhans_debug_builtin_batch records on a second engine of the same weights (whose
    exponents are moved away first); and the fresh engine's exponents are the rule applied to its own maxima."""
    yard, mx, dev = _open(*case)
    assert dev.base == C.expected_exponents(dev.amax0, [0] * 25), (dev.base, dev.amax0)
    assert all(m > 0 and np.isfinite(m) for m in dev.amax0)
    mixes, ca, cb = hip.builtin_batch()
    other = engine.Engine(yard.kind, yard.W, precision="f16x3")
    try:
        assert other.activation_exponents() == dev.base and other.activation_amax() == dev.amax0       # (deterministic)
        other.set_activation_exponents([e + 7 for e in dev.base])
        mix_t, moff = other._dev(mixes)
        ca_t, caoff = other._dev(ca)
        cb_t, cboff = other._dev(cb)
        other.set_precision("f32")
        other.set_option("calibrate", 1)
        try:
            other.enhance_device(mix_t, moff, ca_t, caoff, cb_t, cboff)
        except BaseException:
            other.set_option("calibrate", 3)
            raise
        other.set_option("calibrate", 0)
        other.set_precision("f16x3")
        amax, E = other.activation_amax(), other.activation_exponents()
        assert other.take_status() == 0
    finally:
        other.close()
    print("\n%s %s: built-in maxima %s\nexponents %s" % (case + (["%.6g" % m for m in dev.amax0], dev.base)))
    assert amax == dev.amax0, [(j, a, b) for j, (a, b) in enumerate(zip(amax, dev.amax0)) if a != b]
    assert E == dev.base, (E, dev.base)
