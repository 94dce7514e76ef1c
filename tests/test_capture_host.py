"""Conditioning captured from a slot's own stream, the parts that need no device: the new names in the header, the
binding and the library; nhans_capture_plan and online.ring_runs against a numpy ring; the vlo rule (online.capture_vlo /
capture_span) against a simulated ring over random sequences of push, rewind, restart and enable."""
import ctypes
import os
import re

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import hip, live, online, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 32240
NAMES = ("nhans_capture_plan", "nhans_capture_enable", "nhans_capture_context", "nhans_capture_embeddings",
         "nhans_capture_live_enable", "nhans_capture_live_context", "nhans_capture_live_embeddings")


@pytest.fixture(scope="module")
def lib(lib_built):
    return hip.load()


def test_names_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void) (nhans_capture_\w+)\(", text, re.M))
    assert declared == set(NAMES) == {n for n in hip.EXPORTS if n.startswith("nhans_capture_")}
    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        getattr(lib, n)
    assert lib.nhans_abi_version() == 5 == hip.ABI_VERSION and re.search(r"#define NHANS_ABI_VERSION 5\b", text)
    for name, value in (("NHANS_CAPTURE_SAMPLES", hip.CAPTURE_SAMPLES), ("NHANS_CAPTURE_A", hip.CAPTURE_A),
                        ("NHANS_CAPTURE_B", hip.CAPTURE_B), ("NHANS_CAPTURE_NORMALISE", hip.CAPTURE_NORMALISE)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert hip.CAPTURE_SAMPLES == online.CAPTURE_SAMPLES == CAP == (spec.NOISE_WIN - 1) * spec.HOP + spec.WIN
    assert int(re.search(r"#define NHANS_ESHORT \((-\d+)\)", text).group(1)) == hip.ESHORT
    for cls in (online.OnlineEnhancer, live.LiveSession):
        for m in ("enable_capture", "capture_context", "capture_contexts", "embeddings"):
            assert callable(getattr(cls, m)), m
    # a NULL object is refused before anything touches a device, with the function's name in the message
    for n in NAMES[1:]:
        f = getattr(lib, n)
        args = {"enable": (None, None), "context": (None, 1, None, None, 0, None, None), "embeddings": (None, 0, None, None, None)}
        assert f(*args[n.rsplit("_", 1)[1]]) == -1
        assert n.encode() in lib.nhans_last_error()


def test_sides_follow_the_model_kind():
    assert [online.capture_side("denoiser", w) for w in ("a", "b", "pos", "neg", 0, 1)] == [0, 1, 0, 1, 0, 1]
    assert [online.capture_side("separator", w) for w in ("a", "b", "pos", "neg")] == [0, 1, 1, 0]
    for bad in ("c", 2, None):
        with pytest.raises(ValueError, match="which"):
            online.capture_side("denoiser", bad)


def _plan(lib, n_before, count):
    out = (ctypes.c_int64 * 6)(*([-1] * 6))
    n = lib.nhans_capture_plan(n_before, count, out)
    assert 0 <= n <= 2, (n_before, count, n)
    return [tuple(out[3 * r:3 * r + 3]) for r in range(n)]


N_BEFORE = [0, 1, 32239, 32240, 32241, 64479, 64480]
COUNTS = [0, 1, 159, 160, 161, 8191, 8192, 8193, 32239, 32240, 32241, 40000]


def test_plan_against_a_numpy_ring(lib):
    """Brute force: a ring that holds x[max(0, n - CAP) : n] at positions k mod CAP holds x[max(0, N - CAP) : N] the same
    way after the runs of a push of `count` samples, N = n + count; the runs neither overlap nor leave the ring nor the
    push; a count of 0 gives none; the Python restatement agrees with the C function."""
    rng = np.random.default_rng(5)
    befores = N_BEFORE + [int(v) for v in rng.integers(0, 200000, 12)]
    x = np.arange(200000 + 40000, dtype=np.int64)            # the stream: sample k has value k
    for n in befores:
        base = np.full(CAP, -1, np.int64)
        k = np.arange(max(0, n - CAP), n)
        base[k % CAP] = x[k]
        for count in COUNTS:
            runs = _plan(lib, n, count)
            assert runs == online.ring_runs(n, count), (n, count)
            if count == 0:
                assert runs == []
                continue
            ring = base.copy()
            push = x[n:n + count]
            hit = np.zeros(CAP, np.int32)
            for off, pos, length in runs:
                assert length > 0 and 0 <= off and off + length <= count and 0 <= pos and pos + length <= CAP, (n, count, runs)
                ring[pos:pos + length] = push[off:off + length]
                hit[pos:pos + length] += 1
            assert hit.max() == 1 and hit.sum() == min(count, CAP), (n, count)
            N = n + count
            k = np.arange(max(0, N - CAP), N)
            assert np.array_equal(ring[k % CAP], x[k]), (n, count)
    assert lib.nhans_capture_plan(-1, 5, (ctypes.c_int64 * 6)()) == -1 and b"nhans_capture_plan" in lib.nhans_last_error()
    assert lib.nhans_capture_plan(5, -1, (ctypes.c_int64 * 6)()) == -1
    assert lib.nhans_capture_plan(5, 1, None) == -1 and lib.nhans_capture_plan(5, 0, None) == 0
    with pytest.raises(ValueError):
        online.ring_runs(0, -1)


class _Slot:
    """One slot of an online object as the header describes it, with content identities in place of samples: `truth[k]`
    is the identity of sample k of the current stream, `ring` what the device ring would hold (-1: never written)."""

    def __init__(self):
        self.ids = 0
        self.truth = np.zeros(0, np.int64)
        self.ring = None
        self.vlo = None
        self.undone = None          # (ids, n_before) of a rewound push: the redo pushes the same input
        self.last = None            # (ids, n_before) of the last push while it can still be rewound

    @property
    def N(self):
        return len(self.truth)

    def enable(self):
        if self.ring is None:
            self.ring = np.full(CAP, -1, np.int64)
            self.vlo = online.capture_vlo(self.vlo, "enable", self.N)

    def push(self, count):
        if self.undone is not None:                         # the saturation redo: the same push with the same input
            new = self.undone[0]
            self.undone = None
        else:
            new = np.arange(self.ids, self.ids + count, dtype=np.int64)
            self.ids += count
        n = self.N
        if self.ring is not None:
            for off, pos, length in online.ring_runs(n, len(new)):
                self.ring[pos:pos + length] = new[off:off + length]
        self.truth = np.concatenate([self.truth, new])
        if self.ring is not None:
            self.vlo = online.capture_vlo(self.vlo, "push", self.N)
        self.last = (new, n)

    def rewind(self):
        if self.last is None:
            return
        new, n = self.last
        hN = self.N
        self.truth = self.truth[:n]
        if self.ring is not None:
            self.vlo = online.capture_vlo(self.vlo, "rewind", hN)
        self.undone, self.last = self.last, None

    def restart(self):
        self.truth = np.zeros(0, np.int64)
        self.undone = self.last = None
        if self.ring is not None:
            self.vlo = online.capture_vlo(self.vlo, "restart", 0)

    def valid(self):
        """Every sample of [N - CAP, N) in the ring is the one pushed on the current timeline."""
        if self.ring is None or self.N < CAP:
            return False
        k = np.arange(self.N - CAP, self.N)
        return bool(np.array_equal(self.ring[k % CAP], self.truth[k]))


def test_vlo_rule_against_a_simulated_ring():
    """Random sequences of push, rewind, restart and enable (a rewound push is repeated with the same input by the slot's
    next push, which is what the rewind exists for; the history is enabled at any time except between a push and its
    rewind): online.capture_span(N, vlo) is a span exactly when the simulated ring holds the last CAP samples of the
    current stream, and then it is [N - CAP, N)."""
    rng = np.random.default_rng(17)
    sizes = [0, 1, 160, 3000, 8193, 20000, 32239, 32240, 32241, 40000]
    seen = {True: 0, False: 0}
    for seq in range(40):
        s = _Slot()
        if seq % 2 == 0:
            s.enable()
        for step in range(40):
            ev = rng.choice(["push", "push", "push", "push", "rewind", "restart", "enable"], p=[.2, .2, .2, .2, .1, .04, .06])
            if ev == "push":
                s.push(int(rng.choice(sizes)))
            elif ev == "enable" and s.last is not None:
                continue                                    # (the one ordering where the rule is only safe: see below)
            else:
                getattr(s, ev)()
            if s.ring is None:
                continue
            span = online.capture_span(s.N, s.vlo)
            assert (span is not None) == s.valid(), (seq, step, ev, s.N, s.vlo)
            if span is not None:
                assert span == (s.N - CAP, s.N)
            seen[span is not None] += 1
    assert min(seen.values()) > 50, seen
    # history enabled between a push and its rewind: vlo = N of that moment lies above the rewound stream, and the rule
    # stays on the safe side -- no span although the repeated push has filled the ring -- for one ring length
    s = _Slot()
    s.push(40000)
    s.enable()
    s.rewind()
    s.push(40000)
    assert s.valid() and online.capture_span(s.N, s.vlo) is None
    s.push(CAP)
    assert s.valid() and online.capture_span(s.N, s.vlo) == (40000, 40000 + CAP)
    assert online.capture_span(CAP - 1, 0) is None and online.capture_span(CAP, 0) == (0, CAP)
    assert online.capture_span(42239, 10000) is None and online.capture_span(42240, 10000) == (10000, 42240)
    with pytest.raises(ValueError):
        online.capture_vlo(0, "other", 0)
