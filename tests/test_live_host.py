"""Live PCM sessions, the parts that need no device: the output contract nhans_live_emitted of include/nhans_hip.h
against its Python restatement live.emitted (the three stages' contracts chained), and the new names in the header, the
binding and the library."""
import os
import re

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nhans_live_emitted", "nhans_live_open_slots", "nhans_live_restart", "nhans_live_set_context",
         "nhans_live_set_embeddings", "nhans_live_set_wet", "nhans_live_out_counts", "nhans_live_push", "nhans_live_rewind",
         "nhans_live_close"]


@pytest.fixture(scope="module")
def lib(lib_built):
    return hip.load()


def _ns():
    rng = np.random.default_rng(2024)
    return list(range(6001)) + sorted(int(v) for v in rng.integers(6001, 10 ** 6 + 1, 300))


@pytest.mark.parametrize("rate_in", resample.RATES)
def test_emitted_is_the_chained_contract(lib, rate_in):
    """Every (in, out) combination, 16000 on both sides included, every n in 0 ... 6,000 and 300 seeded n up to 1e6,
    ended and not: C == Python, and the value never decreases with n."""
    ns = _ns()
    for rate_out in resample.RATES:
        for ended in (False, True):
            last = 0
            for n in ns:
                got = lib.nhans_live_emitted(n, int(ended), rate_in, rate_out)
                assert got == live.emitted(n, ended, rate_in, rate_out), (n, ended, rate_in, rate_out)
                assert got >= last, (n, ended, rate_in, rate_out)
                last = got


@pytest.mark.parametrize("rate_in", resample.RATES)
def test_an_ended_stream_has_the_offline_length(lib, rate_in):
    """Ended: the conversion of the 16 kHz recording trimmed to whole frames -- apply.trim_to_frames on an array of the
    converted length, then resample.out_count."""
    rng = np.random.default_rng(rate_in)
    for n in [0, 1, 399, 400, 1199, 1200, 1201] + [int(v) for v in rng.integers(0, 200000, 40)]:
        n16 = resample.out_count(n, rate_in, 16000)
        trimmed = len(apply.trim_to_frames(np.zeros(n16, np.float32))) if n16 >= 400 else 0
        for rate_out in resample.RATES:
            assert lib.nhans_live_emitted(n, 1, rate_in, rate_out) == resample.out_count(trimmed, 16000, rate_out)


def test_a_running_stream_waits_for_every_stage(lib):
    """Not ended: nothing before the 17-frame look-ahead is there, and never more than the ended value."""
    for rate_in, rate_out in ((48000, 48000), (44100, 16000), (16000, 44100), (8000, 96000)):
        first = (17 * 160 + 400) * rate_in // 16000
        assert lib.nhans_live_emitted(first - rate_in // 100, 0, rate_in, rate_out) == 0
        for n in range(0, 4 * rate_in, rate_in // 7):
            assert lib.nhans_live_emitted(n, 0, rate_in, rate_out) <= lib.nhans_live_emitted(n, 1, rate_in, rate_out)
    assert online.emitted(resample.emitted(48000, False, 48000, 16000), False) == 160 * 80


def test_unsupported_rates_name_both(lib):
    for pair in ((44000, 48000), (48000, 7000), (0, 16000), (16000, -1)):
        assert lib.nhans_live_emitted(100, 0, *pair) == -1
        msg = lib.nhans_last_error()
        assert b"nhans_live_emitted" in msg and str(pair[0]).encode() in msg and str(pair[1]).encode() in msg
        with pytest.raises(ValueError):
            live.emitted(100, False, *pair)
    assert lib.nhans_live_emitted(-1, 0, 48000, 48000) == -1
    assert lib.nhans_live_emitted(48000, 0, 44100, 48000) > 0           # (neither side 16000: both stages convert)


def test_the_live_functions_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void) (nhans_live_\w+)\(", text, re.M))
    assert declared == set(NAMES) == {n for n in hip.EXPORTS if n.startswith("nhans_live_")}
    for n in NAMES:
        getattr(lib, n)
    assert lib.nhans_abi_version() == 5 and re.search(r"#define NHANS_ABI_VERSION 5\b", text)
    assert re.search(r"#define NHANS_LIVE_WET %d\b" % hip.LIVE_WET, text)
    for m in ("restart", "set_context", "set_embeddings", "set_wet", "out_counts", "push", "push_device", "rewind", "close"):
        assert callable(getattr(live.LiveSession, m)), m
    assert live.default_out_scale(21000, np.int16) == 21000 + 1e-6 and live.default_out_scale(21000, np.float32) == 1.0
