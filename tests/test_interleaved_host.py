"""Interleaved live sessions without a device: the nhans_interleaved_* names of the header against the binding and the
library, the mode constants, the ABI number, and live.downmix -- the numpy statement of the sample a downmix session
forms from a frame -- against exact rational arithmetic."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np

import nhans_amd  # noqa: F401
from nhans_amd import hip, live

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nhans_interleaved_live_open", "nhans_interleaved_live_out_counts", "nhans_interleaved_live_push"]


def _header():
    return open(os.path.join(ROOT, "include", "nhans_hip.h")).read()


def test_names_are_the_headers_the_bindings_and_the_librarys(lib_built):
    declared = set(re.findall(r"\b(nhans_interleaved_[a-z_0-9]+)\s*\(", _header()))
    assert declared == set(NAMES) == {n for n in hip.EXPORTS if n.startswith("nhans_interleaved_")}
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert len(hip.SIGNATURES["nhans_interleaved_live_open"][1]) == 14
    assert hip.SIGNATURES["nhans_interleaved_live_push"] == hip.SIGNATURES["nhans_live_push"]
    assert hip.SIGNATURES["nhans_interleaved_live_out_counts"] == hip.SIGNATURES["nhans_live_out_counts"]


def test_mode_macros_equal_the_bindings_constants():
    macros = dict(re.findall(r"#define (NHANS_INTERLEAVED_[A-Z_]+) (\d+)", _header()))
    assert macros == {"NHANS_INTERLEAVED_DOWNMIX": str(hip.INTERLEAVED_DOWNMIX), "NHANS_INTERLEAVED_SPLIT": str(hip.INTERLEAVED_SPLIT),
                      "NHANS_INTERLEAVED_MAX_CHANNELS": str(hip.INTERLEAVED_MAX_CHANNELS)}
    assert hip.INTERLEAVED_DOWNMIX != hip.INTERLEAVED_SPLIT and hip.INTERLEAVED_MAX_CHANNELS == 8
    assert live.CHANNEL_MODES == {"downmix": hip.INTERLEAVED_DOWNMIX, "split": hip.INTERLEAVED_SPLIT}


def test_abi_version_is_5(lib_built):
    assert re.search(r"#define NHANS_ABI_VERSION (\d+)", _header()).group(1) == "5"
    assert hip.load().nhans_abi_version() == hip.ABI_VERSION == 5


def test_null_objects_are_refused_by_name(lib_built):
    lib = hip.load()
    out = (ctypes.c_int64 * 1)()
    assert lib.nhans_interleaved_live_push(None, None, None, None, None, None, out, None) == -1
    assert b"nhans_interleaved_live_push" in lib.nhans_last_error()
    assert lib.nhans_interleaved_live_out_counts(None, out, None, out) == -1
    assert b"nhans_interleaved_live_out_counts" in lib.nhans_last_error()
    assert lib.nhans_interleaved_live_open(None, 1, 2, 2, 0, 48000, 0, 1.0, 48000, 0, 1.0, 0, None, None) == -1
    assert b"nhans_interleaved_live_open" in lib.nhans_last_error()


def _exact(frames):
    """float32 nearest (ties to even) to the exact rational mean of each int16 frame: the double sum of <= 8 int16 values
    is exact, the double quotient is the correctly rounded one, and what is checked here is that rounding it again to
    float32 is harmless -- the mean of C <= 8 integers below 2^18 in magnitude is a multiple of 1 / C, and float64 holds
    it to 2^-35 relative, far inside the gap between a float32 and the nearest float32 tie for C in 1 .. 8."""
    out = np.empty(len(frames), dtype=np.float32)
    for k, f in enumerate(frames):
        q = Fraction(sum(int(v) for v in f), len(f))
        lo = np.float32(float(q))                         # a candidate; step to its neighbours and keep the nearest
        best = min((np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))),
                   key=lambda v: (abs(Fraction(float(v)) - q), int(v.view(np.uint32)) & 1))
        out[k] = best
    return out


def test_downmix_is_the_exact_rational_mean_for_int16():
    rng = np.random.default_rng(5)
    for C in range(1, 9):
        x = rng.integers(-32768, 32768, size=(400, C)).astype(np.int16)
        x[0], x[1], x[2] = 32767, -32768, 0
        x[3, :] = [(-1) ** c * 32767 for c in range(C)]
        got = live.downmix(x)
        assert got.dtype == np.float32 and got.shape == (400,)
        assert got.tobytes() == _exact(x).tobytes(), C


def test_downmix_adds_in_channel_order():
    # float32 frames where the order of a double sum matters: (2^60 + 1) - 2^60 = 0, (2^60 - 2^60) + 1 = 1
    x = np.array([[2.0 ** 60, 1.0, -(2.0 ** 60)], [2.0 ** 60, -(2.0 ** 60), 1.0]], dtype=np.float32)
    assert live.downmix(x).tolist() == [0.0, np.float32(1.0 / 3.0)]


def test_downmix_of_one_channel_is_the_identity():
    rng = np.random.default_rng(6)
    i16 = rng.integers(-32768, 32768, size=1000).astype(np.int16)
    assert np.array_equal(live.downmix(i16), i16.astype(np.float32))
    assert np.array_equal(live.downmix(i16[:, None]), i16.astype(np.float32))
    f32 = np.concatenate([rng.standard_normal(1000).astype(np.float32) * np.float32(1e-3),
                          np.array([np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1e-45, -1.5], dtype=np.float32)])
    got = live.downmix(f32[:, None])
    assert got.dtype == np.float32 and got.tobytes() == f32.tobytes()
