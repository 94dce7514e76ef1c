"""Filterbank features, the part that needs no device (include/nhans_hip.h: nhans_fbank_*): the names, the triangular
designer against this file's own numpy restatement (tests/fbank_checks.py), what the designer and nhans_fbank_open refuse,
and that the float64 bar of the device tests can see a filterbank that is one bin off."""
import ctypes
import os
import re

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import fbank, hip, spec

import fbank_checks as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)


def test_names_and_abi(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(nhans_fbank_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted(n for n in hip.EXPORTS if n.startswith("nhans_fbank_"))
    assert declared == sorted(["nhans_fbank_design", "nhans_fbank_open", "nhans_fbank_close", "nhans_fbank_rows",
                               "nhans_fbank_online_attach", "nhans_fbank_online_read", "nhans_fbank_live_attach",
                               "nhans_fbank_live_read"])
    lib = hip.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.nhans_abi_version() == hip.ABI_VERSION == 5
    assert int(re.search(r"#define NHANS_ABI_VERSION (\d+)", header).group(1)) == 5
    # declared before nhans_profile_json: hip.SIGNATURES follows the header's order
    names = list(hip.SIGNATURES)
    assert max(names.index(n) for n in declared) < names.index("nhans_profile_json")
    for name, value in (("NHANS_FBANK_MAX_OUT", hip.FBANK_MAX_OUT), ("NHANS_FBANK_MAX_SPAN", hip.FBANK_MAX_SPAN),
                        ("NHANS_FBANK_HTK", hip.FBANK_HTK), ("NHANS_FBANK_SLANEY", hip.FBANK_SLANEY),
                        ("NHANS_FBANK_NORM_NONE", hip.FBANK_NORM_NONE), ("NHANS_FBANK_NORM_SLANEY", hip.FBANK_NORM_SLANEY),
                        ("NHANS_FBANK_MIXED", hip.FBANK_MIXED)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value, name


@pytest.mark.parametrize("scale", ["htk", "slaney"])
@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("n,f_min,f_max", [(23, 0.0, 8000.0), (40, 0.0, 8000.0), (80, 0.0, 8000.0), (128, 0.0, 8000.0),
                                           (40, 300.0, 3400.0), (128, 300.0, 3400.0)])
def test_designer_against_the_numpy_restatement(lib_built, scale, norm, n, f_min, f_max):
    """Every weight within 1e-12 of its band's peak height (1, or 2 / (p[m+2] - p[m]) under the Slaney norm): a few
    thousand double roundings; a misplaced edge is off by >= 1e-3 of it.  The empty-band count is the restatement's."""
    W, empty = fbank.design(n, f_min, f_max, scale, norm)
    want, p, peak = F.np_design(n, f_min, f_max, scale, norm)
    assert W.shape == want.shape == (n, spec.BINS) and W.dtype == np.float64
    assert np.all(W >= 0) and np.all(np.isfinite(W))
    assert np.all(np.abs(W - want) <= 1e-12 * peak[:, None]), float(np.max(np.abs(W - want) / peak[:, None]))
    assert empty == F.empty_bands(want)
    if (f_min, f_max) == (0.0, 8000.0):
        # (no band is empty at full range -- except 128 HTK bands: the HTK scale puts them 13.7 Hz apart at 0 Hz, so the
        # lowest triangles are 27 Hz wide and four of them fall between two bins 40 Hz apart; the Slaney scale, linear at
        # 66.7 Hz per mel below 1 kHz, has none)
        assert empty == (4 if (scale, n) == ("htk", 128) else 0)
    assert p[0] == pytest.approx(f_min, abs=1e-9) and p[-1] == pytest.approx(f_max, abs=1e-9)
    # the count alone, without a matrix
    assert hip.load().nhans_fbank_design(n, f_min, f_max, fbank.SCALES[scale], fbank.NORMS[norm], None) == empty
    fb = fbank.Filterbank(n, f_min, f_max, scale, norm)
    assert np.array_equal(fb.matrix, W) and fb.empty_bands == empty and fb.n_mels == n


def test_narrow_bands_are_counted_empty(lib_built):
    """128 bands on 300 - 3400 Hz are narrower than the 40 Hz between bins at the low end: some hold no bin, the designer
    says how many, and such a band's feature is ln(floor)."""
    W, empty = fbank.design(128, 300.0, 700.0, "htk", None)
    assert empty == F.empty_bands(F.np_design(128, 300.0, 700.0, "htk", None)[0]) > 0
    fb = fbank.Filterbank(128, 300.0, 700.0)
    ref = fb.reference(F.uniform_rows(3))
    dead = fb.spans()[1] == 0
    assert dead.sum() == empty and np.all(ref[:, dead] == np.log(np.float64(np.float32(1e-10))))


def test_designer_refusals_change_nothing(lib_built):
    lib = hip.load()
    buf = np.full(129 * spec.BINS, -7.0)
    ptr = buf.ctypes.data_as(_dp)
    ok = (40, 0.0, 8000.0, hip.FBANK_HTK, hip.FBANK_NORM_NONE)
    bad = [(0,) + ok[1:], (129,) + ok[1:], (40, -1.0, 8000.0) + ok[3:], (40, 0.0, 8000.5) + ok[3:], (40, 4000.0, 4000.0) + ok[3:],
           (40, 5000.0, 4000.0) + ok[3:], (40, float("nan"), 8000.0) + ok[3:], ok[:3] + (2, 0), ok[:3] + (-1, 0), ok[:3] + (0, 2),
           ok[:3] + (0, -1)]
    for args in bad:
        assert lib.nhans_fbank_design(*args, ptr) == -1, args
        assert b"nhans_fbank_design" in lib.nhans_last_error()
        assert np.all(buf == -7.0), args
    assert lib.nhans_fbank_design(*ok, ptr) == 0 and np.all(buf[:40 * spec.BINS] >= 0) and np.all(buf[40 * spec.BINS:] == -7.0)
    with pytest.raises(ValueError):
        fbank.Filterbank(40, scale="bark")
    with pytest.raises(ValueError):
        fbank.Filterbank(40, norm="area")
    with pytest.raises(hip.NhansError):
        fbank.Filterbank(129)
    with pytest.raises(ValueError):
        fbank.Filterbank.from_matrix(np.ones((3, 200)))


def test_open_refuses_the_matrix_before_it_needs_a_device(lib_built):
    """nhans_fbank_open checks the filterbank first (no context is touched: it is NULL here), and a good one then fails on
    the null context -- so every refusal below is the matrix's, by name."""
    lib = hip.load()
    W = np.ascontiguousarray(F.np_design(40, 0.0, 8000.0, "htk", None)[0])

    def open_(w, n, power, floor):
        out = ctypes.c_void_p(1234)
        rc = lib.nhans_fbank_open(None, np.ascontiguousarray(w, dtype=np.float64).ctypes.data_as(_dp), n, power, floor, None,
                                  ctypes.byref(out))
        assert out.value is None                    # (*out is NULL after every failure)
        return rc, lib.nhans_last_error()

    rc, msg = open_(W, 40, 2, 1e-10)
    assert rc == -1 and b"null context" in msg          # the matrix is fine
    for n in (0, 129):
        rc, msg = open_(np.ones((max(n, 1), spec.BINS)), n, 2, 1e-10)
        assert rc == -1 and b"nhans_fbank_open: n_out" in msg
    rc, msg = open_(W, 40, 3, 1e-10)
    assert rc == -1 and b"power must be 1 or 2" in msg
    for floor in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        rc, msg = open_(W, 40, 2, floor)
        assert rc == -1 and b"floor" in msg, floor
    for v in (-1e-9, float("nan"), float("inf"), 1e39):
        B = W.copy()
        B[17, 60] = v
        rc, msg = open_(B, 40, 2, 1e-10)
        assert rc == -1 and b"weight [17, 60]" in msg, v
    rc, msg = open_(np.ones((128, spec.BINS)), 128, 2, 1e-10)     # 25,728 span entries
    assert rc == -1 and b"NHANS_FBANK_MAX_SPAN" in msg and b"25728" in msg
    rc, msg = open_(np.ones((40, spec.BINS)), 40, 2, 1e-10)       # 8,040: under the cap
    assert rc == -1 and b"null context" in msg
    assert lib.nhans_fbank_open(None, None, 40, 2, 1e-10, None, None) == -1
    lib.nhans_fbank_close(None)
    assert lib.nhans_fbank_rows(None, None, 1, None, None) == -1 and b"nhans_fbank_rows" in lib.nhans_last_error()
    assert lib.nhans_fbank_online_attach(None, None, 0) == -1 and lib.nhans_fbank_live_attach(None, None, 0) == -1
    assert lib.nhans_fbank_online_read(None, 0, 0, None, 0, None, None) == -1
    assert lib.nhans_fbank_live_read(None, 0, 0, None, 0, None, None) == -1


def test_reference_restates_the_definition():
    """Filterbank.reference against a loop that follows the header line by line, on the custom bank: spans, the empty
    band, float32 rounding of matrix and floor, the clamp outside the domain."""
    fb = F.bank("custom")
    first, count = fb.spans()
    assert list(first) == [0, 117, 0, 5] and list(count) == [201, 1, 0, 5]
    rows = np.concatenate([F.uniform_rows(4), np.full((1, spec.BINS), 60.0, np.float32)])
    ref = fb.reference(rows)
    W32 = fb.matrix.astype(np.float32)
    for r in range(rows.shape[0]):
        for m in range(fb.n_mels):
            acc = 0.0
            for k in range(first[m], first[m] + count[m]):
                acc += float(W32[m, k]) * np.exp(min(fb.power * float(rows[r, k]), 88.0))
            want = np.log(max(acc, float(np.float32(fb.floor))))
            assert ref[r, m] == pytest.approx(want, rel=1e-13, abs=1e-13)
    assert np.all(np.isfinite(ref))
    assert np.all(ref[:, 2] == np.log(np.float64(np.float32(1e-10))))


@pytest.mark.parametrize("name", ["htk23", "htk40", "htk80", "htk128", "slaney128", "htk40p1"])
def test_the_bar_can_see_a_bank_one_bin_off(lib_built, name):
    """With the bar of the device tests, the reference of the same bank shifted by one bin exceeds 16 x the bar on at
    least half of the elements of the domain batch (numpy on the development machine: a share of 0.88 and more)."""
    fb = F.bank(name) if name in F.BANKS else fbank.Filterbank(int(name[3:]))
    rows = F.uniform_rows(3 * F.TILE + 5)
    ref = fb.reference(rows)
    off = F.shifted(fb).reference(rows)
    share = float(np.mean(np.abs(off - ref) > 16.0 * F.bar(fb, ref)))
    print("%s: share of elements beyond 16 x the bar = %.3f" % (name, share))
    assert F.C_BAR <= 16.0
    assert share >= 0.5
