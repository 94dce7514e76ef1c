"""Slot reuse and live conditioning of online enhancement (nhans_online_open_slots / restart / set_context /
set_embeddings, OnlineEnhancer.open_slots and its methods): recordings that join and leave a running object give exactly
the bits of their solo OFFLINE run (Engine.enhance on the normalised, trimmed recording), a change of conditioning in a
running stream obeys the contract of include/nhans_hip.h bit for bit, rewind and the error codes follow the rules
stated there, and idle slots add no launches."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, online, spec, synth
# (no torch at import time: the torch-free worker below is unpickled from this module in a fresh process)

pytestmark = pytest.mark.gpu

TAIL = 37
EMPTY = np.zeros(0, np.float32)


def _engine(*args, **kw):
    from nhans_amd import engine
    return engine.Engine(*args, **kw)


def _samples(T):
    return spec.WIN + spec.HOP * (T - 1) + TAIL


def _stream(cid, nsamp):
    x = synth.mixture(cid, nsamp / 16000.0 + 0.01)[:nsamp]
    return apply.normalise(x)


def _ctx(cid):
    """Conditioning that differs from caller to caller in both recordings for odd ids, in one for even ids."""
    if cid % 2:
        return apply.normalise(synth.noise_context(cid)), apply.normalise(synth.speaker_context(cid))
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(cid))


def _offline(eng, x, ca, cb):
    m = apply.trim_to_frames(x)
    if len(m) < spec.WIN:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    r = eng.enhance([m], [ca], [cb], want_mixed=True)
    return r["denoised_wav"][0], r["mixed_wav"][0]


def _schedule(rng, n):
    """Piece sizes summing to n: 0- and 1-sample pushes, 399 / 400, whole hops, random sizes."""
    out, left = [], n
    while left > 0:
        k = int(rng.choice([0, 1, 399, 400, 160, 320, int(rng.integers(1, 3000)), int(rng.integers(1, 9000))]))
        k = min(k, left)
        out.append(k)
        left -= k
    return out


class _Caller:
    def __init__(self, cid, nsamp, rng):
        self.x = _stream(cid, nsamp)
        self.ca, self.cb = _ctx(cid)
        self.sched = _schedule(rng, nsamp)
        self.pos = self.step = 0
        self.den, self.mix = [], []
        self.done = False

    def next_piece(self):
        k = self.sched[self.step]
        self.step += 1
        piece = self.x[self.pos:self.pos + k]
        self.pos += k
        return piece, self.step == len(self.sched)

    def out(self):
        return (np.concatenate(self.den) if self.den else EMPTY), (np.concatenate(self.mix) if self.mix else EMPTY)


def _round(enh, seats):
    """One push: every seated caller that is not done pushes its next piece, every other slot pushes nothing.  Counts are
    checked against the Python formula and nhans_online_out_counts, as tests/test_gpu_online.py does."""
    chunks, end = [EMPTY] * enh.S, [False] * enh.S
    for i, c in seats.items():
        if not c.done:
            chunks[i], end[i] = c.next_piece()
    n = [len(c) for c in chunks]
    want = online.out_counts(list(enh.pushed), n, end, list(enh.ended))
    assert enh.out_counts(n, end) == want
    outs = enh.push(chunks, end)
    for i in range(enh.S):
        assert len(outs[i][0]) == want[i]
        if i not in seats:
            assert want[i] == 0
            continue
        seats[i].den.append(outs[i][0])
        seats[i].mix.append(outs[i][1])
        seats[i].done = seats[i].done or end[i]
        assert enh.ended[i] == seats[i].done


def _join(enh, seats, slot, caller):
    enh.restart(slot)
    assert enh.pushed[slot] == 0 and enh.ended[slot] is False
    assert enh.set_context(slot, caller.ca, caller.cb) == 0          # a fresh stream: every frame uses the new rows
    assert enh.conditioned[slot] is True
    seats[slot] = caller


@pytest.mark.parametrize("kind,prec", [("denoiser", "f16x3"), ("separator", "f32")], ids=["den-f16x3", "sep-f32"])
def test_slots_are_reused_by_callers_that_join_and_leave(lib_built, weights_denoiser, weights_separator, kind, prec):
    """Three slots, five callers.  A (40 frames) and B (120 frames) join at once, C (1 frame) after three pushes; A ends
    with `end` and D (< 400 samples) takes its slot with other conditioning; B is abandoned by restart while it runs and
    E (305 frames) takes its slot.  A, C, D, E equal their solo offline runs bit for bit, denoised and mixed; B equals
    the first 160 * P samples of its offline run."""
    eng = _engine(kind, weights_denoiser if kind == "denoiser" else weights_separator, precision=prec)
    rng = np.random.default_rng(11)
    A, B, C = _Caller(901, _samples(40), rng), _Caller(902, _samples(120), rng), _Caller(903, _samples(1), rng)
    D, E = _Caller(904, 250, rng), _Caller(905, _samples(305), rng)
    enh = online.OnlineEnhancer.open_slots(eng, 3, want_mixed=True)
    assert enh.conditioned == [False] * 3 and enh.pushed == [0] * 3 and enh.ended == [False] * 3
    seats = {}
    _join(enh, seats, 0, A)
    _join(enh, seats, 1, B)
    rounds = 0
    b_cut = None
    while not all(c.done for c in (A, C, D, E)) or b_cut is None:
        _round(enh, seats)
        rounds += 1
        assert rounds < 2000
        if rounds == 3:
            _join(enh, seats, 2, C)
        if A.done and seats[0] is A:
            _join(enh, seats, 0, D)
        if b_cut is None and B.pos > 8000:
            assert not B.done                                       # abandoned while it runs: its tail is dropped
            b_cut = enh.first_new_frame(1) & ~1                     # P of B's stream at that moment
            _join(enh, seats, 1, E)
    enh.close()
    for name, c in (("A", A), ("C", C), ("D", D), ("E", E)):
        den, mix = c.out()
        rd, rm = _offline(eng, c.x, c.ca, c.cb)
        assert np.array_equal(den, rd), name
        assert np.array_equal(mix, rm), name
    assert len(D.out()[0]) == 0 and len(C.out()[0]) == spec.WIN
    den, mix = B.out()
    rd, rm = _offline(eng, B.x, B.ca, B.cb)
    assert b_cut > 0 and len(den) == spec.HOP * b_cut
    assert np.array_equal(den, rd[:spec.HOP * b_cut]) and np.array_equal(mix, rm[:spec.HOP * b_cut])
    eng.close()


def test_restart_keeps_the_conditioning_of_an_opened_object(lib_built, weights_denoiser):
    """An object from nhans_online_open: after a stream that ended and after one that was still running, a restart gives
    a stream whose output equals the offline run with the contexts the object was opened with."""
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    ca, cb = _ctx(911)
    enh = online.OnlineEnhancer(e, [ca], [cb], want_mixed=True)
    assert enh.conditioned == [True]
    x1, x2, x3 = _stream(911, _samples(50)), _stream(912, _samples(44)), _stream(913, _samples(23))
    (d1, m1), = enh.push([x1], end=[True])
    assert np.array_equal(d1, _offline(e, x1, ca, cb)[0])
    enh.restart(0)
    assert enh.pushed == [0] and enh.ended == [False] and enh.out_counts([_samples(19)]) == [2 * spec.HOP]
    a = enh.push([x2[:5000]])[0]
    b = enh.push([x2[5000:]], end=[True])[0]
    r = _offline(e, x2, ca, cb)
    assert np.array_equal(np.concatenate([a[0], b[0]]), r[0]) and np.array_equal(np.concatenate([a[1], b[1]]), r[1])
    enh.restart(0)
    enh.push([x1[:6000]])                                             # left running, then abandoned
    enh.restart(0)
    (d3, m3), = enh.push([x3], end=[True])
    r = _offline(e, x3, ca, cb)
    assert np.array_equal(d3, r[0]) and np.array_equal(m3, r[1])
    enh.close()
    e.close()


def test_set_embeddings_with_rows_of_engine_embed_equals_set_context(lib_built, weights_denoiser):
    import torch
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    ca, cb = _ctx(921)
    x = _stream(921, _samples(70))
    wav = torch.from_numpy(np.concatenate([ca, cb])).to(e.device)
    lm, _ = e.stft_features(wav, [0, len(ca), len(ca) + len(cb)], max_frames=spec.NOISE_WIN, want_phase=False)
    rows = e.embed(lm.reshape(2, spec.NOISE_WIN, spec.BINS))
    outs = []
    for how in ("context", "device rows", "host rows"):
        enh = online.OnlineEnhancer.open_slots(e, 2, want_mixed=True)
        if how == "context":
            assert enh.set_context(1, ca, cb) == 0
        elif how == "device rows":
            assert enh.set_embeddings(1, rows[0], rows[1]) == 0
        else:
            assert enh.set_embeddings(1, rows[0].cpu().numpy(), rows[1].cpu().numpy()) == 0
        assert enh.conditioned == [False, True]
        p = enh.push([EMPTY, x[:7000]])[1]
        q = enh.push([EMPTY, x[7000:]], end=[False, True])[1]
        outs.append((np.concatenate([p[0], q[0]]), np.concatenate([p[1], q[1]])))
        enh.close()
    r = _offline(e, x, ca, cb)
    for d, m in outs:
        assert d.tobytes() == r[0].tobytes() and m.tobytes() == r[1].tobytes()
    with pytest.raises(ValueError):
        online.OnlineEnhancer.open_slots(e, 1).set_embeddings(0, np.zeros(511, np.float32), np.zeros(512, np.float32))
    e.close()


T_CHANGE = 61


@pytest.mark.parametrize("R", [0, 7, 12, T_CHANGE], ids=["R0", "R-odd", "R-even", "R-final"])
def test_change_of_conditioning_in_a_running_stream_obeys_the_contract(lib_built, weights_denoiser, R):
    """set_context in the middle of a stream of 61 frames, at a point where R frames have been computed (R = 61: after
    `end`).  The call reports R; samples [0, 160 B) are den1 and samples [160 B' + 240, end) are den2 bit for bit, what
    lies between is finite, mixed is the offline one.  den1 and den2 are checked to differ in the last hop before the
    old bound and in the first hop after the new one, so that neither comparison can pass on equal references."""
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    x = _stream(931, _samples(T_CHANGE))
    ca1, cb1 = _ctx(932)
    ca2, cb2 = _ctx(933)
    den1, mix1 = _offline(e, x, ca1, cb1)
    den2, mix2 = _offline(e, x, ca2, cb2)
    assert np.array_equal(mix1, mix2)
    enh = online.OnlineEnhancer.open_slots(e, 2, want_mixed=True)
    enh.set_context(0, ca1, cb1)
    if R == T_CHANGE:
        n1, end1 = len(x), True
    else:
        n1, end1 = spec.WIN + spec.HOP * (R + online.LOOKAHEAD - 1) + 5, False      # T = R + 17 frames pushed
    p = enh.push([x[:n1], EMPTY], end=[end1, False])[0]
    assert enh.first_new_frame(0) == R
    assert enh.set_context(0, ca2, cb2) == R
    q = enh.push([x[n1:], EMPTY], end=[not end1, False])[0]
    enh.close()
    den, mix = np.concatenate([p[0], q[0]]), np.concatenate([p[1], q[1]])
    assert mix.tobytes() == mix1.tobytes()
    assert len(den) == len(den1) == len(den2)
    lo, hi = online.change_bounds(R)
    assert (lo, hi) == (spec.HOP * (R & ~1), spec.HOP * (R + (R & 1)) + 240)
    if R == 0:
        assert den.tobytes() == den2.tobytes() and not np.array_equal(den1, den2)
    elif R == T_CHANGE:
        assert den.tobytes() == den1.tobytes() and not np.array_equal(den1, den2)
    else:
        assert 0 < lo < hi < len(den) - spec.HOP and hi - lo <= 560
        assert not np.array_equal(den1[lo - spec.HOP:lo], den2[lo - spec.HOP:lo])
        assert not np.array_equal(den1[hi:hi + spec.HOP], den2[hi:hi + spec.HOP])
        assert den[:lo].tobytes() == den1[:lo].tobytes()
        assert den[hi:].tobytes() == den2[hi:].tobytes()
        assert np.isfinite(den[lo:hi]).all()
    e.close()


def test_rewind_rules_with_restart_and_set_calls(lib_built, weights_denoiser):
    """restart / set_context / set_embeddings make the last push final; push, rewind, the same push gives the same bytes
    on an object with idle slots; restart, push, rewind, push gives the NEW stream's bytes."""
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    ca, cb = _ctx(941)
    x, y = _stream(941, _samples(80)), _stream(942, _samples(48))
    enh = online.OnlineEnhancer.open_slots(e, 3)
    enh.set_context(1, ca, cb)
    with pytest.raises(hip.NhansError, match="rewind"):
        enh.rewind()
    push = lambda piece, end=False: enh.push([EMPTY, piece, EMPTY], end=[False, end, False])[1][0]
    push(x[:3000])
    enh.restart(2)
    with pytest.raises(hip.NhansError, match="rewind"):
        enh.rewind()
    assert enh.pushed == [0, 3000, 0]
    push(x[3000:6000])
    enh.set_context(0, ca, cb)
    with pytest.raises(hip.NhansError, match="rewind"):
        enh.rewind()
    push(x[6000:7000])
    row = np.zeros(spec.EMB, np.float32)
    enh.set_embeddings(2, row, row)
    with pytest.raises(hip.NhansError, match="rewind"):
        enh.rewind()
    assert enh.pushed == [0, 7000, 0]
    d1 = push(x[7000:11000])
    enh.rewind()
    assert enh.pushed == [0, 7000, 0]
    d2 = push(x[7000:11000])
    assert len(d1) > 0 and d1.tobytes() == d2.tobytes()
    ref_x = _offline(e, x, ca, cb)[0]
    assert np.array_equal(d2, ref_x[online.emitted(7000, False):online.emitted(11000, False)])
    # the stream of x is replaced by that of y: a rewind after y's first push goes back to y's start, not to x
    enh.restart(1)
    y1 = push(y[:5000])
    enh.rewind()
    assert enh.pushed == [0, 0, 0] and enh.ended == [False] * 3
    y2 = push(y[:5000])
    y3 = push(y[5000:], end=True)
    assert len(y1) > 0 and y1.tobytes() == y2.tobytes()
    assert np.array_equal(np.concatenate([y2, y3]), _offline(e, y, ca, cb)[0])
    enh.close()
    e.close()


def test_slot_errors_come_back_as_codes_and_change_nothing(lib_built, weights_denoiser):
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    lib = hip.load()
    err = lambda: lib.nhans_last_error().decode()
    ca, cb = _ctx(951)
    ca2, cb2 = _ctx(952)
    x = _stream(951, _samples(64))
    ref = _offline(e, x, ca, cb)[0]
    enh = online.OnlineEnhancer.open_slots(e, 2)
    dev = enh.mem.up(np.concatenate([ca2, cb2]))
    pa = ctypes.c_void_p(dev.data_ptr())
    pb = ctypes.c_void_p(dev.data_ptr() + 4 * len(ca2))
    R = ctypes.c_int64(-7)
    for slot in (-1, 2):
        assert lib.nhans_online_restart(enh.handle, slot) == -1 and "nhans_online_restart" in err()
        assert lib.nhans_online_set_context(enh.handle, slot, pa, len(ca2), pb, len(cb2), None, ctypes.byref(R)) == -1
        assert "nhans_online_set_context" in err()
        assert lib.nhans_online_set_embeddings(enh.handle, slot, pa, pb, None, ctypes.byref(R)) == -1
        assert "nhans_online_set_embeddings" in err()
    assert lib.nhans_online_restart(None, 0) == -1 and "nhans_online_restart" in err()
    assert lib.nhans_online_set_context(None, 0, pa, len(ca2), pb, len(cb2), None, None) == -1
    assert "nhans_online_set_context" in err()
    assert lib.nhans_online_set_embeddings(None, 0, pa, pb, None, None) == -1 and "nhans_online_set_embeddings" in err()
    assert lib.nhans_online_set_context(enh.handle, 0, None, len(ca2), pb, len(cb2), None, None) == -1
    assert "nhans_online_set_context" in err()
    assert lib.nhans_online_set_embeddings(enh.handle, 0, pa, None, None, None) == -1
    assert "nhans_online_set_embeddings" in err()
    h = ctypes.c_void_p()
    assert lib.nhans_online_open_slots(e.handle, 0, 0, None, ctypes.byref(h)) == -1 and "nhans_online_open_slots" in err()
    assert lib.nhans_online_open_slots(e.handle, 2, 0, None, None) == -1 and "nhans_online_open_slots" in err()
    assert lib.nhans_online_open_slots(None, 2, 0, None, ctypes.byref(h)) < 0
    assert R.value == -7 and enh.conditioned == [False, False]
    # an unconditioned slot takes 0-sample pushes and nothing else
    assert [len(d) for d, _ in enh.push([EMPTY, EMPTY])] == [0, 0]
    with pytest.raises(hip.NhansError, match="no conditioning") as ei:
        enh.push([x[:1000], EMPTY])
    assert "(code -1)" in str(ei.value)
    with pytest.raises(hip.NhansError, match="no conditioning"):
        enh.push([EMPTY, EMPTY], end=[False, True])
    assert enh.pushed == [0, 0] and enh.ended == [False, False]
    # a refused change of conditioning on a running stream: the stream goes on under the old one
    enh.set_context(0, ca, cb)
    a = enh.push([x[:6000], EMPTY])[0][0]
    with pytest.raises(hip.NhansError) as ei:
        enh.set_context(0, ca2[:32239], cb2)
    assert "(code -4)" in str(ei.value)                                    # NHANS_ESHORT
    with pytest.raises(hip.NhansError) as ei:
        enh.set_context(0, ca2, cb2[:32239])
    assert "(code -4)" in str(ei.value)
    assert enh.pushed == [6000, 0] and enh.conditioned == [True, False]
    b = enh.push([x[6000:], EMPTY], end=[True, False])[0][0]
    assert np.array_equal(np.concatenate([a, b]), ref)
    enh.close()
    e.close()


def test_idle_slots_add_no_launches(lib_built, weights_denoiser):
    """Eight slots with two active against a two-stream nhans_online_open object, the same pushes: equal output bytes
    and equal per-kernel launch counts in nhans_profile_json."""
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    xs = [_stream(961, _samples(45)), _stream(962, _samples(30))]
    ctx = [_ctx(961), _ctx(962)]
    pieces = [(0, 0), (1500, 0), (2500, 4000), (3000, 900)]
    where = {2: 0, 5: 1}                                               # slot -> stream

    def run(enh, slot_of):
        e.set_option("profile", 1)
        e.profile_reset()
        pos, outs = [0, 0], [[], []]
        steps = pieces + [(len(xs[0]), len(xs[1]))]
        for k, n in enumerate(steps):
            chunks, end = [EMPTY] * enh.S, [False] * enh.S
            for j in range(2):
                chunks[slot_of[j]] = xs[j][pos[j]:pos[j] + n[j]]
                end[slot_of[j]] = k == len(steps) - 1
                pos[j] += n[j]
            res = enh.push(chunks, end)
            for j in range(2):
                outs[j].append(res[slot_of[j]][0])
        prof = e.profile()
        e.set_option("profile", 0)
        enh.close()
        return [np.concatenate(o) for o in outs], {k: v["calls"] for k, v in prof.items()}

    fixed = online.OnlineEnhancer(e, [c[0] for c in ctx], [c[1] for c in ctx])
    out_f, calls_f = run(fixed, [0, 1])
    slots = online.OnlineEnhancer.open_slots(e, 8)
    for s, j in where.items():
        slots.set_context(s, *ctx[j])
    out_s, calls_s = run(slots, [2, 5])
    assert calls_f == calls_s and sum(calls_f.values()) > 0 and "online_istft" in calls_f
    for j in range(2):
        assert out_f[j].tobytes() == out_s[j].tobytes()
        assert np.array_equal(out_s[j], _offline(e, xs[j], *ctx[j])[0])
    e.close()


def _lite_worker(q):
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        os.environ["NHANS_NO_TORCH"] = "1"
        import nhans_amd  # noqa: F401
        from nhans_amd import apply, lite, online, synth, weights
        le = lite.LiteEngine("denoiser", weights.synthetic_weights("denoiser", 7))
        xs = [apply.normalise(synth.mixture(971, 1.1)), apply.normalise(synth.mixture(972, 0.9))]
        ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(971))
        enh = online.OnlineEnhancer.open_slots(le, 2, want_mixed=True)
        out = []
        for x, (a, b) in zip(xs, ((ca, cb), (cb, ca))):               # the second caller reuses slot 1, contexts swapped
            enh.restart(1)
            first = enh.set_context(1, a, b)
            den, mix = [], []
            for i in range(0, len(x), 1234):
                (_, _), (d, m) = enh.push([np.zeros(0, np.float32), x[i:i + 1234]], end=[False, i + 1234 >= len(x)])
                den.append(d); mix.append(m)
            out.append((np.concatenate(den), np.concatenate(mix), first))
        cond = list(enh.conditioned)
        enh.close()
        le.close()
        q.put((out, cond, "torch" in sys.modules, None))
    except Exception as e:
        import traceback
        q.put((None, None, None, traceback.format_exc() + repr(e)))


def test_torch_free_slots_equal_the_offline_engine(lib_built):
    from nhans_amd import weights
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_lite_worker, args=(q,))
    p.start()
    try:
        out, cond, had_torch, err = q.get(timeout=600)
    finally:
        p.join(timeout=120)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert had_torch is False and cond == [False, True]
    e = _engine("denoiser", weights.synthetic_weights("denoiser", 7), precision="f16x3")
    xs = [apply.normalise(synth.mixture(971, 1.1)), apply.normalise(synth.mixture(972, 0.9))]
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(971))
    for (den, mix, first), x, (a, b) in zip(out, xs, ((ca, cb), (cb, ca))):
        r = _offline(e, x, a, b)
        assert first == 0 and np.array_equal(den, r[0]) and np.array_equal(mix, r[1])
    e.close()
