"""context.py without a device: the exact sequence of calls redo_saturated_in_f32 makes on an engine, for every way a
batch or push can go, and the look-ahead bracket of Context on a recording handle."""
import warnings

import pytest

import nhans_amd  # noqa: F401
from nhans_amd import context, hip, spec


class FakeEngine:
    """Records every set_option / set_precision / take_status call (and, through run / undo below, those too).
    status: what the take_status calls return (an exception: raise), in order; fail: {logged call: the exception that call
    raises}."""

    def __init__(self, status, precision="f16x3", fail=None):
        self.log = []
        self.precision = precision
        self.status = list(status)
        self.fail = fail or {}

    def _call(self, *entry):
        self.log.append(entry)
        if entry in self.fail:
            raise self.fail[entry]

    def set_option(self, key, value):
        self._call("set_option", key, value)

    def set_precision(self, name):
        self._call("set_precision", name)
        self.precision = name

    def take_status(self):
        self._call("take_status")
        status = self.status.pop(0)
        if isinstance(status, BaseException):
            raise status
        return status

    def run(self):
        n = 1 + sum(e[0] == "run" for e in self.log)
        self._call("run", n)
        return "result %d" % n

    def undo(self):
        self._call("undo")


SAT = hip.STATUS_SATURATED
REDO = [("set_option", "calibrate", 1), ("set_precision", "f32"), ("run", 2), ("take_status",)]


def test_a_clean_run_is_one_run_and_one_status():
    eng = FakeEngine([0])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert context.redo_saturated_in_f32(eng, eng.run, eng.undo) == "result 1"
    assert eng.log == [("run", 1), ("take_status",)]


def test_other_status_bits_are_not_saturation():
    eng = FakeEngine([~SAT])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert context.redo_saturated_in_f32(eng, eng.run) == "result 1"
    assert eng.log == [("run", 1), ("take_status",)]


def test_saturation_in_f32_mode_is_left_alone():
    eng = FakeEngine([SAT], precision="f32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert context.redo_saturated_in_f32(eng, eng.run, eng.undo) == "result 1"
    assert eng.log == [("run", 1), ("take_status",)] and eng.precision == "f32"


@pytest.mark.parametrize("with_undo", [False, True])
def test_saturation_in_f16x3_redoes_the_work_in_f32(with_undo):
    eng = FakeEngine([SAT, 0])
    with pytest.warns(UserWarning, match="f16 range") as seen:
        res = context.redo_saturated_in_f32(eng, eng.run, eng.undo if with_undo else None)
    assert res == "result 2" and len(seen) == 1
    assert eng.log == [("run", 1), ("take_status",)] + ([("undo",)] if with_undo else []) + REDO + [
        ("set_option", "calibrate", 2), ("set_precision", "f16x3")]
    assert eng.precision == "f16x3"


@pytest.mark.parametrize("exc", [RuntimeError("second run"), KeyboardInterrupt()])
def test_a_failing_redo_closes_the_bracket_then_restores_the_precision(exc):
    eng = FakeEngine([SAT], fail={("run", 2): exc})
    with pytest.warns(UserWarning, match="f16 range"), pytest.raises(type(exc)) as ei:
        context.redo_saturated_in_f32(eng, eng.run, eng.undo)
    assert ei.value is exc
    assert eng.log == [("run", 1), ("take_status",), ("undo",)] + REDO[:3] + [
        ("set_option", "calibrate", 3), ("set_precision", "f16x3")]
    assert ("set_option", "calibrate", 2) not in eng.log and eng.precision == "f16x3"


def test_a_failing_status_after_the_redo_counts_as_a_failing_redo():
    exc = hip.NhansError("take_status")
    eng = FakeEngine([SAT, exc])
    with pytest.warns(UserWarning, match="f16 range"), pytest.raises(hip.NhansError) as ei:
        context.redo_saturated_in_f32(eng, eng.run)
    assert ei.value is exc
    assert eng.log == [("run", 1), ("take_status",)] + REDO + [("set_option", "calibrate", 3), ("set_precision", "f16x3")]


def test_the_precision_comes_back_even_if_closing_the_bracket_fails():
    eng = FakeEngine([SAT], fail={("run", 2): RuntimeError("second run"),
                                  ("set_option", "calibrate", 3): hip.NhansError("calibrate 3")})
    with pytest.warns(UserWarning, match="f16 range"), pytest.raises(hip.NhansError, match="calibrate 3") as ei:
        context.redo_saturated_in_f32(eng, eng.run, eng.undo)
    assert str(ei.value.__context__) == "second run"              # (the original error is still there to read)
    assert eng.log[-2:] == [("set_option", "calibrate", 3), ("set_precision", "f16x3")] and eng.precision == "f16x3"
    assert ("set_option", "calibrate", 2) not in eng.log


def test_the_f32_result_stands_if_the_exponent_update_fails():
    eng = FakeEngine([SAT, 0], fail={("set_option", "calibrate", 2): hip.NhansError("no finite maximum")})
    with pytest.warns(UserWarning) as seen:
        res = context.redo_saturated_in_f32(eng, eng.run, eng.undo)
    assert res == "result 2"
    assert ["f16 range" in str(w.message) for w in seen] == [True, False]
    assert "exponents not updated" in str(seen[1].message) and "no finite maximum" in str(seen[1].message)
    assert eng.log == [("run", 1), ("take_status",), ("undo",)] + REDO + [
        ("set_option", "calibrate", 2), ("set_precision", "f16x3")]
    assert eng.precision == "f16x3"


def test_an_error_other_than_the_librarys_in_the_exponent_update_propagates_with_the_precision_restored():
    eng = FakeEngine([SAT, 0], fail={("set_option", "calibrate", 2): KeyboardInterrupt()})
    with pytest.warns(UserWarning, match="f16 range"), pytest.raises(KeyboardInterrupt):
        context.redo_saturated_in_f32(eng, eng.run)
    assert eng.log[-2:] == [("set_option", "calibrate", 2), ("set_precision", "f16x3")]


# ---- the look-ahead bracket of Context, on a handle that records its option calls ---------------------------------
class FakeLib:
    def __init__(self):
        self.options = []

    def nhans_set_option(self, handle, key, value):
        self.options.append((handle, key, value))
        return 0

    def nhans_destroy(self, handle):
        self.destroyed = handle


def _context():
    ctx = context.Context()
    ctx.lib, ctx.handle = FakeLib(), "handle"
    return ctx


def test_the_default_lookahead_makes_no_option_call():
    ctx = _context()
    assert ctx._with_lookahead(spec.LOOKAHEAD, lambda: "ran") == "ran"
    assert ctx.lib.options == []


def test_another_lookahead_is_set_for_the_run_and_restored():
    ctx = _context()
    seen = []
    assert ctx._with_lookahead(2, lambda: seen.append(list(ctx.lib.options)) or "ran") == "ran"
    assert seen == [[("handle", b"lookahead", 2)]]
    assert ctx.lib.options == [("handle", b"lookahead", 2), ("handle", b"lookahead", spec.LOOKAHEAD)]


def test_the_lookahead_is_restored_when_the_run_raises():
    ctx = _context()

    def run():
        raise RuntimeError("run")

    with pytest.raises(RuntimeError, match="run"):
        ctx._with_lookahead(0, run)
    assert ctx.lib.options == [("handle", b"lookahead", 0), ("handle", b"lookahead", spec.LOOKAHEAD)]


def test_a_lookahead_out_of_range_is_refused_before_any_option_call():
    ctx = _context()
    with pytest.raises(ValueError):
        ctx._with_lookahead(spec.LOOKAHEAD + 1, lambda: "ran")
    assert ctx.lib.options == []


def test_set_precision_keeps_the_name_and_both_engines_are_contexts():
    ctx = _context()
    ctx.set_precision("f32")
    assert ctx.precision == "f32" and ctx.lib.options == [("handle", b"precision", 0)]
    ctx.set_precision("f16x3")
    assert ctx.precision == "f16x3" and ctx.lib.options[-1] == ("handle", b"precision", 1)
    with pytest.raises(KeyError):
        ctx.set_precision("f64")
    assert ctx.precision == "f16x3"
    ctx.close()
    ctx.close()
    assert ctx.lib.destroyed == "handle" and ctx.handle is None
    from nhans_amd import lite
    assert issubclass(lite.LiteEngine, context.Context) and lite.LiteEngine.torch_memory is False
    assert lite.LiteEngine.set_precision is context.Context.set_precision
