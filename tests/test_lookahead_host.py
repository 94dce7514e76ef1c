"""Selectable look-ahead, the parts that need no device: the output contract with look-ahead L (include/nhans_hip.h) as
online.emitted / out_counts / latency_ms restate it, brute force over every T <= 60 x L in 0 ... 17 x ended / not; the
bounds of the carried state of a push (host_internal.h: kOnRows = 42, kOnDenRows = 24) with on_lo / on_s0 restated here;
the live chain against the C function; the header, the binding and the command line's refusals."""
import os
import re

import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX = 60
LS = range(0, 18)
HOPS_PER_BLOCK = 22          # kIstftHopsPerBlock of the iSTFT kernel: synthesis restarts on this grid of a stream's frames
ON_ROWS, ON_DEN_ROWS = 42, 24


def _n(T):
    """Samples of a stream of exactly T frames (T = 0: one sample short of the first)."""
    return spec.WIN + spec.HOP * (T - 1) if T > 0 else spec.WIN - 1


def _closed(T, L, ended):
    """The issue's closed forms: R = max(0, T - L) (T once ended), P = R rounded down to even, 160 P samples; after the
    end (T - 1) * 160 + 400, or 0."""
    if ended:
        return T, T, (0 if T == 0 else (T - 1) * 160 + 400)
    R = max(0, T - L)
    P = R - R % 2
    return R, P, 160 * P


def on_s0(P):
    return max(0, P - 2) // HOPS_PER_BLOCK * HOPS_PER_BLOCK


def on_lo(R, P):
    return max(0, min(R - 17, on_s0(P)))


def test_emitted_matches_the_closed_form_and_is_monotone():
    for L in LS:
        for ended in (False, True):
            last = 0
            for n in range(0, _n(TMAX) + 1):
                T = online.num_frames(n)
                R, P, E = _closed(T, L, ended)
                got = online.emitted(n, ended, lookahead=L)
                assert got == E, (n, L, ended)
                assert online.ready_frames(n, ended, L) == R
                assert got >= last and got <= online.emitted(n, True, lookahead=L), (n, L, ended)
                last = got
    assert online.emitted(_n(20), False, lookahead=2) == 160 * 18 and online.emitted(_n(20), False, lookahead=0) == 160 * 20


def test_lookahead_17_is_the_contract_of_before():
    for n in range(0, _n(TMAX) + 1, 7):
        for ended in (False, True):
            assert online.emitted(n, ended) == online.emitted(n, ended, lookahead=17) == online.emitted(n, ended, 17)
            T = online.num_frames(n)
            R = T if ended else max(0, T - 17)
            want = (0 if T == 0 else (T - 1) * 160 + 400) if ended else 160 * (R - R % 2)
            assert online.emitted(n, ended) == want
    assert online.LOOKAHEAD == spec.LOOKAHEAD == 17
    assert online.out_counts([0, 3000], [5000, 4000], [False, True]) == \
        online.out_counts([0, 3000], [5000, 4000], [False, True], lookahead=17)


def test_out_counts_sum_to_emitted_for_every_cut():
    """Every (T_before, T_after) pair, ended by the push or not: the count is the difference of the totals, never negative,
    and a per-stream list of look-aheads gives each stream its own."""
    for L in LS:
        for Ta in range(0, TMAX + 1, 3):
            for Tb in range(Ta, TMAX + 1, 5):
                for end in (False, True):
                    na, nb = _n(Ta) + 11 * (Ta > 0), _n(Tb) + 11 * (Tb > 0)
                    c, = online.out_counts([na], [nb - na], [end], lookahead=L)
                    assert c == _closed(Tb, L, end)[2] - _closed(Ta, L, False)[2] and c >= 0
    assert online.out_counts([0, 0, 0], [_n(30)] * 3, lookahead=[0, 2, 17]) == [160 * 30, 160 * 28, 160 * 12]
    assert online.out_counts([_n(30)], [0], [True], [True], lookahead=3) == [0]


def test_state_bounds_hold_for_every_lookahead():
    """What a push leaves in a slot: spectrogram rows [lo, T) and denoised rows [S0, R).  T - lo <= max(L + 17, L + 24)
    <= 42 and R - S0 <= 24 for every L <= 17 -- S0 >= P - 23 >= R - 24 and lo >= min(R - 17, S0).  Checked far past
    T = 60 as well: S0 moves on a grid of 22 frames."""
    for L in LS:
        for T in list(range(0, TMAX + 1)) + list(range(61, 400)):
            for ended in (False, True):
                R, P, _ = _closed(T, L, ended)
                lo, s0 = on_lo(R, P), on_s0(P)
                assert T - lo <= ON_ROWS and R - s0 <= ON_DEN_ROWS, (T, L, ended)
                if not ended:
                    assert T - lo <= max(L + 17, L + 24)


def test_latency_follows_the_lookahead():
    for L in LS:
        lo, hi = online.latency_ms(lookahead=L)
        assert abs(lo - (10 * L + 15)) < 1e-9 and abs(hi - (10 * L + 35)) < 1e-9
    assert online.latency_ms() == online.latency_ms(lookahead=17) == (185.0, 205.0)
    assert online.latency_ms(lookahead=2) == (35.0, 55.0) and online.latency_ms(lookahead=0) == (15.0, 35.0)
    a = online.latency_ms(in_rate=48000, out_rate=48000, lookahead=2)
    assert abs(a[0] - 36.25) < 1e-9 and abs(a[1] - 56.25) < 1e-9


def test_change_bounds_is_stated_in_R():
    assert online.change_bounds(0) == (0, 240) and online.change_bounds(7) == (960, 1520)
    assert "ready_frames" in online.change_bounds.__doc__


def test_check_lookahead():
    assert [spec.check_lookahead(L) for L in (0, 2, 17, 3.0)] == [0, 2, 17, 3]
    for bad in (-1, 18, 2.5):
        with pytest.raises(ValueError, match="lookahead"):
            spec.check_lookahead(bad)


@pytest.fixture(scope="module")
def lib(lib_built):
    return hip.load()


def test_live_chain_against_the_library(lib):
    """nhans_lookahead_live_emitted == live.emitted(lookahead=L) for every L, 16 kHz and 48 / 44.1 kHz sides, every n up
    to 60 frames' worth; at L = 17 it is nhans_live_emitted; it never decreases; L outside 0 ... 17 is refused."""
    for rate_in, rate_out in ((16000, 16000), (48000, 48000), (44100, 16000), (16000, 8000)):
        top = _n(TMAX) * rate_in // 16000
        ns = list(range(0, top, 53)) + [top]
        for L in LS:
            for ended in (False, True):
                last = 0
                for n in ns:
                    got = lib.nhans_lookahead_live_emitted(n, int(ended), rate_in, rate_out, L)
                    assert got == live.emitted(n, ended, rate_in, rate_out, lookahead=L), (n, ended, rate_in, rate_out, L)
                    assert got >= last
                    last = got
                    if L == 17:
                        assert got == lib.nhans_live_emitted(n, int(ended), rate_in, rate_out)
    for bad in (-1, 18):
        assert lib.nhans_lookahead_live_emitted(48000, 0, 48000, 48000, bad) == -1
        assert b"lookahead" in lib.nhans_last_error()
    assert lib.nhans_lookahead_live_emitted(48000, 0, 44000, 48000, 2) == -1
    # one second at 48 kHz, L = 2: 98 frames, R = 96 of them ready -- against 80 at the default
    assert online.emitted(15990, False, lookahead=2) == 160 * 96 and online.emitted(15990, False) == 160 * 80


def test_the_new_functions_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "nhans_hip.h")).read()
    for decl in (r"^int nhans_online_set_lookahead\(nhans_online\* obj, int slot, int lookahead\);",
                 r"^int nhans_lookahead_live_set\(nhans_live\* obj, int slot, int lookahead\);",
                 r"^int64_t nhans_lookahead_live_emitted\(int64_t nsamples, int ended, int rate_in, int rate_out, int lookahead\);"):
        assert re.search(decl, text, re.M), decl
    for n in ("nhans_online_set_lookahead", "nhans_lookahead_live_set", "nhans_lookahead_live_emitted"):
        assert n in hip.EXPORTS
        getattr(lib, n)
    assert lib.nhans_abi_version() == 5 == hip.ABI_VERSION and re.search(r"#define NHANS_ABI_VERSION 5\b", text)
    assert '"lookahead"' in text
    assert lib.nhans_online_set_lookahead(None, 0, 2) == -1 and lib.nhans_lookahead_live_set(None, 0, 2) == -1
    for cls, names in ((online.OnlineEnhancer, ("set_lookahead", "open_slots")), (live.LiveSession, ("set_lookahead",))):
        for m in names:
            assert callable(getattr(cls, m)), m


@pytest.mark.parametrize("value", ["175", "15", "-10", "180"])
def test_cli_refuses_what_is_no_whole_frame(value, capsys):
    before = apply.FLAGS.lookahead_ms
    with pytest.raises(SystemExit):
        apply._parse(["--lookahead_ms", value], "nhans_denoiser")
    assert "multiple of 10 in 0 ... 170" in capsys.readouterr().err
    assert apply.FLAGS.lookahead_ms == before == 170


def test_cli_accepts_whole_frames():
    saved = dict(vars(apply.FLAGS))
    try:
        for v, L in (("0", 0), ("20", 2), ("170", 17)):
            a = apply._parse(["--lookahead_ms", v], "nhans_denoiser")
            assert a.lookahead_ms == 10 * L and apply.FLAGS.lookahead_ms == 10 * L
            assert apply._lookahead_kw() == ({} if L == 17 else {"lookahead": L})
        assert apply._parse([], "nhans_separator").lookahead_ms == 170
    finally:
        for k in list(vars(apply.FLAGS)):
            if k not in saved:
                delattr(apply.FLAGS, k)
        for k, v in saved.items():
            setattr(apply.FLAGS, k, v)
