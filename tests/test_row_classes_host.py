"""Row classes of a conv segment (nhans_debug_row_classes, host only): the grouping of output rows by the filter rows
that touch the image, which option row_split launches the 3x3 convs of resblock3 / resblock4 by (host_net.hip:
row_classes, run_conv_row_classes).  Against brute force over the model's own geometries and a sweep."""
import ctypes
import os
import re

import nhans_amd  # noqa: F401
from nhans_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, KH, stride, pt) of the stack's convs that have padding rows: SAME padding, pt = total // 2
MODEL = [(9, 3, 1, 1), (5, 3, 1, 1), (9, 3, 2, 1), (35, 4, 2, 1), (18, 3, 2, 0), (35, 4, 1, 1), (18, 4, 1, 1)]
# the 1x1 stride-2 `_transform` segment under the classes of resblock3_1 / resblock4_1 conv2
TRANSFORM = [(18, 9), (9, 5)]


def classes(lib, H, KH, s, pt, cap=64):
    out = (ctypes.c_int * (4 * cap))()
    n = lib.nhans_debug_row_classes(H, KH, s, pt, out, cap)
    return n, [tuple(out[4 * i:4 * i + 4]) for i in range(max(n, 0))]


def brute(H, KH, s, pt):
    Ho = (H + s - 1) // s
    return [[kh for kh in range(KH) if 0 <= ho * s - pt + kh < H] for ho in range(Ho)]


def check(lib, H, KH, s, pt):
    rows = brute(H, KH, s, pt)
    n, cl = classes(lib, H, KH, s, pt)
    if any(not r for r in rows):
        assert n == 0, (H, KH, s, pt)           # an output row that reads padding only: "do not split"
        return 0
    assert n >= 1, (H, KH, s, pt)
    nxt = 0
    for i, (oh0, nrows, kh0, khn) in enumerate(cl):
        assert oh0 == nxt and nrows >= 1 and khn >= 1, (H, KH, s, pt, cl)       # a partition of [0, Ho), in order
        nxt = oh0 + nrows
        if i:
            assert (kh0, khn) != cl[i - 1][2:], (H, KH, s, pt, cl)              # consecutive rows with one range: one class
        pt_c = pt - kh0 - oh0 * s                                              # the class launch's own top padding
        for r in range(nrows):
            assert rows[oh0 + r] == list(range(kh0, kh0 + khn)), (H, KH, s, pt, cl)
            # the class launch (local row r, filter rows 0 .. khn - 1, padding pt_c) reads the very input rows
            assert [r * s - pt_c + k for k in range(khn)] == [(oh0 + r) * s - pt + kh for kh in rows[oh0 + r]]
    assert nxt == len(rows)
    return n


def test_model_geometries(lib_built):
    lib = hip.load()
    assert classes(lib, 9, 3, 1, 1) == (3, [(0, 1, 1, 2), (1, 7, 0, 3), (8, 1, 0, 2)])
    assert classes(lib, 5, 3, 1, 1) == (3, [(0, 1, 1, 2), (1, 3, 0, 3), (4, 1, 0, 2)])
    assert classes(lib, 9, 3, 2, 1) == (3, [(0, 1, 1, 2), (1, 3, 0, 3), (4, 1, 0, 2)])
    assert classes(lib, 35, 4, 2, 1) == (3, [(0, 1, 1, 3), (1, 16, 0, 4), (17, 1, 0, 2)])
    assert classes(lib, 18, 3, 2, 0) == (2, [(0, 8, 0, 3), (8, 1, 0, 2)])
    for geo in MODEL:
        assert check(lib, *geo) >= 2
    # filter-row applications per frame, before -> after
    applied = lambda H, KH, s, pt: sum(r * k for _, r, _, k in classes(lib, H, KH, s, pt)[1])
    assert [applied(*g) for g in MODEL[:5]] == [25, 13, 13, 69, 26]
    # the `_transform` segment (1x1, stride 2, no padding) under a class that starts at oh0: pt' = -2 oh0, one class of its own
    for H, Ho in TRANSFORM:
        assert classes(lib, H, 1, 2, 0) == (1, [(0, Ho, 0, 1)])
        assert (Ho - 1) * 2 < H                    # its row of the last class is inside the image


def test_sweep_against_brute_force(lib_built):
    lib = hip.load()
    split = none = 0
    for H in range(1, 41):
        for KH in range(1, 9):
            for s in range(1, 4):
                for pt in range(0, KH + 2):        # pt <= KH - 1 is what SAME padding produces; KH and KH + 1 leave a row nothing
                    n = check(lib, H, KH, s, pt)
                    split += n > 0
                    none += n == 0
    assert split > 2000 and none > 500


def test_bad_arguments_and_room(lib_built):
    lib = hip.load()
    out = (ctypes.c_int * 8)()
    assert lib.nhans_debug_row_classes(9, 3, 1, 1, out, 2) == -1 and b"room for 2" in lib.nhans_last_error()
    for bad in [(0, 3, 1, 1), (9, 0, 1, 1), (9, 3, 0, 1), (9, 3, 1, -1)]:
        assert lib.nhans_debug_row_classes(*bad, out, 2) == -1
    assert lib.nhans_debug_row_classes(9, 3, 1, 1, None, 4) == -1
    assert lib.nhans_debug_row_classes(3, 1, 1, 1, None, 0) == 0          # every row reads padding only: nothing to write


def test_symbol_is_declared_bound_and_exported(lib_built):
    header = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"\bint\s+nhans_debug_row_classes\s*\(\s*int H, int KH, int stride, int pt, int\* out, int cap\s*\)\s*;", code)
    restype, argtypes = hip.SIGNATURES["nhans_debug_row_classes"]
    assert restype is ctypes.c_int and len(argtypes) == 6
    assert "nhans_debug_row_classes" in hip.EXPORTS
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "nhans_debug_row_classes")
    assert '"row_split"' in header
