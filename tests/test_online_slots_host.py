"""Slot reuse and live conditioning on the host: online.change_bounds against a brute-force simulation of which output
samples a change of conditioning at frame R can reach (sample -> the frames that cover it -> their iSTFT pair partners),
and the header's new functions in hip.EXPORTS."""
import os
import re

import nhans_amd  # noqa: F401
from nhans_amd import hip, online, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pure_samples(T, R):
    """For a stream of T frames whose frames >= R use the new conditioning: per output sample, whether every frame that
    covers it is 'old-pure' (the frame and its pair partner (2k, 2k+1), if it exists, are both < R) and whether every
    one is 'new-pure' (both >= R).  A frame's waveform bits may depend on its partner's data, nothing else."""
    def partner(t):
        return t ^ 1 if (t ^ 1) < T else None
    old = [t < R and (partner(t) is None or partner(t) < R) for t in range(T)]
    new = [t >= R and (partner(t) is None or partner(t) >= R) for t in range(T)]
    n_out = (T - 1) * spec.HOP + spec.WIN
    s_old, s_new = [], []
    for n in range(n_out):
        cover = [t for t in range(max(0, n // spec.HOP - 3), min(T, n // spec.HOP + 1))
                 if spec.HOP * t <= n < spec.HOP * t + spec.WIN]
        assert cover
        s_old.append(all(old[t] for t in cover))
        s_new.append(all(new[t] for t in cover))
    return s_old, s_new


def test_change_bounds_are_safe_everywhere_and_exact_inside_a_stream():
    for T in range(1, 61):
        for R in range(0, T + 1):
            lo, hi = online.change_bounds(R)
            assert lo == spec.HOP * (R & ~1) and hi == spec.HOP * (R + (R & 1)) + 240 and hi - lo <= 560
            s_old, s_new = _pure_samples(T, R)
            n_out = len(s_old)
            # safe: every sample the contract promises is pure
            assert all(s_old[:min(lo, n_out)]), (T, R)
            assert all(s_new[min(hi, n_out):]), (T, R)
            if R == 0:
                assert all(s_new), (T, R)                      # the whole output is the new conditioning's
            if R == T:
                assert all(s_old), (T, R)                      # ... the old one's
            if 0 < R < T:
                # exact: not one sample more is pure on either side
                assert not any(s_old[lo:]), (T, R)
                assert not any(s_new[:hi]), (T, R)


def test_change_bounds_values():
    assert online.change_bounds(0) == (0, 240)
    assert online.change_bounds(7) == (960, 1520)
    assert online.change_bounds(12) == (1920, 2160)


def test_the_slot_functions_are_declared_bound_and_exported():
    names = ["nhans_online_open_slots", "nhans_online_restart", "nhans_online_set_context", "nhans_online_set_embeddings"]
    text = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    for n in names:
        assert re.search(r"^int %s\(" % n, text, re.M), n
        assert n in hip.EXPORTS, n
    assert hip.ABI_VERSION == 5 and re.search(r"#define NHANS_ABI_VERSION 5\b", text)
    for m in ("open_slots", "restart", "set_context", "set_embeddings"):
        assert callable(getattr(online.OnlineEnhancer, m)), m
