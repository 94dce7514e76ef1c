"""Level meter and automatic compensation of live sessions, the parts that need no device: the hop count
nhans_level_hops of include/nhans_hip.h against its restatement, and the new names in the header, the binding and the
library."""
import os
import re

import pytest

import nhans_amd  # noqa: F401
from nhans_amd import hip, live, online

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nhans_level_hops", "nhans_level_live_enable", "nhans_level_live_auto", "nhans_level_live_read",
         "nhans_level_live_gains", "nhans_level_gains"]


@pytest.fixture(scope="module")
def lib(lib_built):
    return hip.load()


def _hops(emitted, ended):
    if ended:
        return (emitted + 159) // 160
    return emitted // 160


def test_hops_of_every_count_a_short_stream_can_reach(lib):
    """Streams of T <= 60 frames at every look-ahead: running they have emitted 160 * (an even number of ready frames) --
    whole hops --, ended 160 (T + 1) + 80 samples, whose last hop of 80 counts.  C == the three lines above == live.level_hops."""
    seen = set()
    for T in range(61):
        n = 0 if T == 0 else 400 + 160 * (T - 1)
        for L in range(18):
            for ended in (False, True):
                e = online.emitted(n, ended, L)
                seen.add((e, ended))
                if ended:
                    assert e == (160 * (T + 1) + 80 if T else 0)
                    assert _hops(e, True) == (T + 2 if T else 0)
                else:
                    assert e % 320 == 0 and _hops(e, False) * 160 == e
    assert len(seen) > 90
    for e, ended in sorted(seen):
        assert lib.nhans_level_hops(e, int(ended)) == _hops(e, ended) == live.level_hops(e, ended), (e, ended)
    assert lib.nhans_level_hops(-1, 0) == -1 and b"nhans_level_hops" in lib.nhans_last_error()
    with pytest.raises(ValueError):
        live.level_hops(-1, False)
    # (any count, not only reachable ones: a whole clip of the offline twin ends wherever it ends)
    for e in (1, 79, 80, 159, 160, 161, 319, 2 ** 40 + 1):
        assert lib.nhans_level_hops(e, 1) == _hops(e, True) and lib.nhans_level_hops(e, 0) == _hops(e, False)


def test_the_level_functions_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void) (nhans_level_\w+)\(", text, re.M))
    assert declared == set(NAMES) == {n for n in hip.EXPORTS if n.startswith("nhans_level_")}
    for n in NAMES:
        getattr(lib, n)
    assert lib.nhans_abi_version() == 5 and re.search(r"#define NHANS_ABI_VERSION 5\b", text)
    for m in ("enable_levels", "set_auto_wet", "levels", "last_gains"):
        assert callable(getattr(live.LiveSession, m)), m
    assert callable(live.level_gains)


def test_null_objects_are_refused_by_name(lib):
    import ctypes
    out = (ctypes.c_double * 8)()
    for call, name in ((lambda: lib.nhans_level_live_enable(None, None), b"nhans_level_live_enable"),
                       (lambda: lib.nhans_level_live_auto(None, 4, 1.0), b"nhans_level_live_auto"),
                       (lambda: lib.nhans_level_live_read(None, 0, out, None), b"nhans_level_live_read"),
                       (lambda: lib.nhans_level_live_gains(None, 0, None, 0, None), b"nhans_level_live_gains")):
        assert call() == -1 and name in lib.nhans_last_error()
