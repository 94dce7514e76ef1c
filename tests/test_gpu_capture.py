"""Conditioning captured from a slot's own stream (include/nhans_hip.h: nhans_capture_*; OnlineEnhancer / LiveSession
enable_capture, capture_context(s), embeddings): the captured row is bit for bit the tower row of the last 32,240 samples
the slot received -- however the stream was cut, alone or in a batch, as stored or peak-normalised, at 16 kHz and behind
the incoming converter of a live session --, it acts on the stream as set_embeddings with that row does, the vlo rule
answers NHANS_ESHORT where the ring does not hold the span, and a push costs the launches it cost before."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, resample, spec, synth
# (no torch at import time: the torch-free worker below is unpickled from this module in a fresh process)

pytestmark = pytest.mark.gpu

CAP = online.CAPTURE_SAMPLES
EMPTY = np.zeros(0, np.float32)
NTOT = 50000
PEAK = 20000.0
EMB_TOL = 2e-5          # tests/test_gpu_recipes.py: tower rows against the float64 oracle on identical float32 features


def _engine(*args, **kw):
    from nhans_amd import engine
    return engine.Engine(*args, **kw)


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


_cache = {}


def _x():
    """The seeded recording of 50,000 normalised samples every 16 kHz test pushes: computed once, never written to."""
    if "x" not in _cache:
        x = apply.normalise(synth.mixture(941, NTOT / 16000.0 + 0.01)[:NTOT])
        assert x.dtype == np.float32 and len(x) == NTOT
        x.setflags(write=False)
        _cache["x"] = x
    return _cache["x"]


def _ctx():
    if "ctx" not in _cache:
        _cache["ctx"] = (apply.normalise(synth.silent()), apply.normalise(synth.noise_context(941)))
    return _cache["ctx"]


def _features(e, clip):
    import torch
    clip = np.array(clip, dtype=np.float32)                      # (a writable copy: the shared recording is read-only)
    assert len(clip) == CAP
    lm, _ = e.stft_features(torch.from_numpy(clip).to(e.device), [0, CAP], max_frames=spec.NOISE_WIN, want_phase=False)
    return lm.reshape(1, spec.NOISE_WIN, spec.BINS)


def _row(e, clip):
    """engine.embed(engine.stft_features(clip, max_frames=200)): the row nhans_online_set_context stores for the clip."""
    return e.embed(_features(e, clip))[0].cpu().numpy()


def _peak_normalised(clip):
    """nhans_peak_normalise with flags 0 on the host: float32(double(x) / (double(max|x|) + 1e-6))."""
    return online.normalise_fixed(clip, float(np.abs(np.asarray(clip, np.float32)).max()))


def _start_rows(e):
    """The rows every object of these tests starts from: the tower rows of the two context recordings."""
    if "rows" not in _cache:
        ca, cb = _ctx()
        _cache["rows"] = (_row(e, ca[:CAP]), _row(e, cb[:CAP]))
    return _cache["rows"]


def _open(e, S, capture=True, **kw):
    enh = online.OnlineEnhancer.open_slots(e, S, **kw)
    a, b = _start_rows(e)
    for i in range(S):
        enh.set_embeddings(i, a, b)
    if capture:
        enh.enable_capture()
    return enh


def _push_to(enh, x, targets):
    """One push that brings slot i to targets[i] samples of x."""
    enh.push([x[enh.pushed[i]:targets[i]] for i in range(enh.S)])
    assert enh.pushed == list(targets)


def _code(ei):
    return ei.value.code


def _eq(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape == (spec.EMB,) and np.array_equal(a, b)


def test_rows_do_not_depend_on_the_cutting(eng):
    """Three slots, one recording, three cuttings -- one push; pieces of 1 / 159 / 160 / 161 / 5,000 / 0; 9,760 then
    40,240 (more than the ring holds): row b as stored is the same in all three and equals the tower row of
    x[17,760:50,000]; row a is untouched."""
    x = _x()
    cuts = [[NTOT], [], [9760, 40240]]
    while sum(cuts[1]) < NTOT:
        for k in (1, 159, 160, 161, 5000, 0):
            cuts[1].append(min(k, NTOT - sum(cuts[1])))
    enh = _open(eng, 3)
    try:
        pos = [0, 0, 0]
        for r in range(max(len(c) for c in cuts)):
            chunks = []
            for i in range(3):
                k = cuts[i][r] if r < len(cuts[i]) else 0
                chunks.append(x[pos[i]:pos[i] + k])
                pos[i] += k
            enh.push(chunks)
        assert enh.pushed == [NTOT] * 3
        want_R = online.ready_frames(NTOT, False)
        for i in range(3):
            assert enh.capture_context(i, "b", normalise=False) == want_R
        rows = [enh.embeddings(i) for i in range(3)]
    finally:
        enh.close()
    want = _row(eng, x[NTOT - CAP:])
    a0, b0 = _start_rows(eng)
    for a, b in rows:
        assert _eq(b, want) and _eq(a, a0)
    assert not np.array_equal(want, b0)


def test_normalised_equals_set_context_of_the_normalised_slice(eng):
    x = _x()
    clip = _peak_normalised(x[NTOT - CAP:])
    assert not np.array_equal(clip, x[NTOT - CAP:])
    enh, twin = _open(eng, 1), _open(eng, 1, capture=False)
    try:
        _push_to(enh, x, [NTOT])
        enh.capture_context(0, "neg", normalise=True)               # denoiser: neg is side b
        twin.set_context(0, clip, clip)
        got, ref = enh.embeddings(0), twin.embeddings(0)
    finally:
        enh.close()
        twin.close()
    assert _eq(got[1], ref[1]) and _eq(ref[0], ref[1]) and _eq(got[0], _start_rows(eng)[0])


def test_edges_of_the_span(eng):
    """N = 32,239: NHANS_ESHORT; 32,240: the ring exactly full, no wrap; 32,241: wrapped by one.  History enabled after
    10,000 samples: NHANS_ESHORT until N >= 42,240, then the row of x[10,000:42,240]."""
    x = _x()
    enh, late = _open(eng, 1), _open(eng, 1, capture=False)
    try:
        _push_to(enh, x, [CAP - 1])
        before = enh.embeddings(0)
        with pytest.raises(hip.NhansError, match="nhans_capture_context.*samples so far") as ei:
            enh.capture_context(0, "b", normalise=False)
        assert _code(ei) == hip.ESHORT
        assert all(_eq(u, v) for u, v in zip(enh.embeddings(0), before))
        for n in (CAP, CAP + 1):
            _push_to(enh, x, [n])
            enh.capture_context(0, "b", normalise=False)
            assert _eq(enh.embeddings(0)[1], _row(eng, x[n - CAP:n])), n

        with pytest.raises(hip.NhansError, match="not enabled") as ei:
            late.capture_context(0, "b")
        assert _code(ei) == -1
        _push_to(late, x, [10000])
        late.enable_capture()
        late.enable_capture()                                       # idempotent
        _push_to(late, x, [10000 + CAP - 1])
        with pytest.raises(hip.NhansError, match="enabled at sample 10000") as ei:
            late.capture_context(0, "b", normalise=False)
        assert _code(ei) == hip.ESHORT
        _push_to(late, x, [10000 + CAP])
        late.capture_context(0, "b", normalise=False)
        assert _eq(late.embeddings(0)[1], _row(eng, x[10000:10000 + CAP]))
    finally:
        enh.close()
        late.close()


def test_batch_equals_one_call_each(eng):
    x = _x()
    targets = [33000, 40000, NTOT]
    pairs = [(0, "a"), (1, "b"), (2, "b"), (2, "a")]
    enh, twin = _open(eng, 3), _open(eng, 3)
    try:
        for o in (enh, twin):
            _push_to(o, x, targets)
        R = enh.capture_contexts(pairs)
        R1 = [twin.capture_context(i, w) for i, w in pairs]
        assert R == R1 == [online.ready_frames(targets[i], False) for i, _ in pairs]
        rows = [enh.embeddings(i) for i in range(3)]
        for i in range(3):
            assert all(_eq(u, v) for u, v in zip(rows[i], twin.embeddings(i))), i
        a0, b0 = _start_rows(eng)
        assert _eq(rows[0][1], b0) and _eq(rows[1][0], a0)
        assert _eq(rows[1][1], _row(eng, _peak_normalised(x[targets[1] - CAP:targets[1]])))
        for bad, msg in (([(1, "a"), (0, "b"), (1, "a")], "named twice"), ([(3, "a")], "slot 3"), ([], "n must be")):
            with pytest.raises(hip.NhansError, match="nhans_capture_context.*" + msg) as ei:
                enh.capture_contexts(bad)
            assert _code(ei) == -1
        for i in range(3):
            assert all(_eq(u, v) for u, v in zip(rows[i], enh.embeddings(i))), i
        lib = hip.load()
        import ctypes
        one = (ctypes.c_int * 1)(0)
        assert lib.nhans_capture_context(enh.handle, 1, one, (ctypes.c_int * 1)(2), 0, None, None) == -1
        assert lib.nhans_capture_context(enh.handle, 1, one, one, 2, None, None) == -1
        assert b"unknown flag" in lib.nhans_last_error()
        assert lib.nhans_capture_context(enh.handle, 1, None, one, 0, None, None) == -1
    finally:
        enh.close()
        twin.close()


def test_effect_on_the_stream_is_that_of_set_embeddings(eng):
    """A captures side b after the push that brought 40,000 samples; B gets set_embeddings(a row, tower row of the
    normalised slice) at the same point: the same R, every later push bit-identical, and against the offline runs under
    the old and the new conditioning the change_bounds regions hold bit for bit."""
    x = _x()
    ca, cb = _ctx()
    k = 40000
    clip = _peak_normalised(x[k - CAP:k])
    A, B = _open(eng, 1), _open(eng, 1, capture=False)
    try:
        outs = {}
        for name, o in (("A", A), ("B", B)):
            parts = [o.push([x[:k]])[0][0]]
            if name == "A":
                R = o.capture_context(0, "b")
            else:
                R2 = o.set_embeddings(0, _start_rows(eng)[0], _row(eng, clip))
            for a, b in ((k, 43000), (43000, 43001), (43001, NTOT)):
                parts.append(o.push([x[a:b]], end=[b == NTOT])[0][0])
            outs[name] = parts
    finally:
        A.close()
        B.close()
    assert R == R2 == online.ready_frames(k, False)
    assert all(np.array_equal(u, v) for u, v in zip(outs["A"], outs["B"]))
    m = apply.trim_to_frames(x)
    r = eng.enhance([m, m], [ca[:CAP], ca[:CAP]], [cb[:CAP], clip], want_mixed=False)
    den1, den2 = r["denoised_wav"]
    got = np.concatenate(outs["A"])
    lo, hi = online.change_bounds(R)
    assert len(got) == len(den1) and 0 < lo < hi < len(got)
    assert np.array_equal(got[:lo], den1[:lo]) and np.array_equal(got[hi:], den2[hi:])
    assert not np.array_equal(den1[hi:], den2[hi:])


def test_rewind(eng):
    x = _x()
    enh, twin = _open(eng, 1), _open(eng, 1)
    try:
        for o in (enh, twin):
            _push_to(o, x, [40000])
            _push_to(o, x, [45000])
        enh.rewind()
        before = enh.embeddings(0)
        with pytest.raises(hip.NhansError, match="rewound") as ei:
            enh.capture_context(0, "b", normalise=False)
        assert _code(ei) == hip.ESHORT
        assert all(_eq(u, v) for u, v in zip(enh.embeddings(0), before))
        _push_to(enh, x, [45000])                                   # the same push with the same input: the saturation redo
        assert enh.capture_context(0, "b", normalise=False) == twin.capture_context(0, "b", normalise=False)
        assert all(_eq(u, v) for u, v in zip(enh.embeddings(0), twin.embeddings(0)))
        assert _eq(enh.embeddings(0)[1], _row(eng, x[45000 - CAP:45000]))
        with pytest.raises(hip.NhansError, match="nhans_online_rewind") as ei:
            enh.rewind()                                            # a capture makes the last push final, as a set call does
        assert _code(ei) == -1
    finally:
        enh.close()
        twin.close()


def _recording_48k():
    """2.3 s on the int16 scale at 48 kHz, with a tail that fills no hop."""
    return np.ascontiguousarray(np.repeat(synth.mixture(943, 2.3), 3)[:-101].astype(np.int16))


def _live_rows(e):
    x = _recording_48k()
    sess = live.LiveSession(e, 2, 48000, 48000, PEAK)
    try:
        ca, cb = _ctx()
        sess.set_context(1, ca, cb)
        sess.enable_capture()
        for a, b in ((0, 4801), (4801, 4802), (4802, 60000), (60000, len(x))):
            sess.push([np.zeros(0, np.int16), x[a:b]])
        R = sess.capture_contexts([(1, "neg")], normalise=True)
        start = sess.embeddings(1)
        R += sess.capture_contexts([(1, "a")], normalise=False)
        return R, start, sess.embeddings(1)
    finally:
        sess.close()


def _lite_worker(q):
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        os.environ["NHANS_NO_TORCH"] = "1"
        import nhans_amd  # noqa: F401
        from nhans_amd import lite, weights
        le = lite.LiteEngine("denoiser", weights.synthetic_weights("denoiser", 7))
        out = _live_rows(le)
        le.close()
        q.put((out, "torch" in sys.modules, None))
    except Exception as e:
        import traceback
        q.put((None, None, traceback.format_exc() + repr(e)))


def test_live_48k_int16_equals_the_offline_chain(eng):
    """Rows captured in a live session are those of the offline chain: nhans_resample of everything pushed, division by
    peak + 1e-6, the last 32,240 of the first nhans_resample_emitted(...) samples, (peak normalisation,) STFT, tower --
    over Engine and, in a process without torch, over LiteEngine."""
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_lite_worker, args=(q,))
    p.start()
    try:
        R, start, rows = _live_rows(eng)
        x = _recording_48k()
        n16 = resample.emitted(len(x), False, 48000, 16000)
        y = online.normalise_fixed(resample.resample(eng, [x], 48000, 16000)[0], PEAK)[:n16]
        assert n16 > CAP and _lib_n16(len(x)) == n16
        clip = y[n16 - CAP:]
        ca, cb = _ctx()
        assert R == [online.ready_frames(n16, False)] * 2
        assert _eq(start[1], _row(eng, _peak_normalised(clip))) and _eq(start[0], _row(eng, ca[:CAP]))
        assert _eq(rows[0], _row(eng, clip)) and _eq(rows[1], start[1])
        out, had_torch, err = q.get(timeout=600)
    finally:
        p.join(timeout=120)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert had_torch is False
    assert out[0] == R
    for got, want in zip(out[1] + out[2], start + rows):
        assert _eq(got, want)


def _lib_n16(n48):
    return hip.load().nhans_resample_emitted(n48, 0, 48000, 16000)


def _calls(e, fn):
    e.set_option("profile", 1)
    e.profile_reset()
    try:
        fn()
        return {k: v["calls"] for k, v in e.profile().items()}
    finally:
        e.set_option("profile", 0)


def test_cost_structure(eng):
    """A push issues the same launches with the history enabled as without; a one-entry capture issues the kernels of
    set_context plus exactly one capture_clip_kernel, and nothing of the stack or of a push."""
    x = _x()
    ca, cb = _ctx()
    on, off = _open(eng, 2), _open(eng, 2, capture=False)
    try:
        for o in (on, off):
            o.push([x[:33000], x[:2000]])
        prof = [_calls(eng, lambda o=o: o.push([x[33000:33480], x[2000:2480]])) for o in (on, off)]
        assert prof[0] == prof[1] and prof[0]["online_ingest"] == 1 and "cond_proj" in prof[0]
        big = [_calls(eng, lambda o=o: o.push([x[33480:NTOT], EMPTY])) for o in (on, off)]
        assert big[0] == big[1]
        cap = _calls(eng, lambda: on.capture_context(0, "b"))
        ctx = _calls(eng, lambda: off.set_context(0, ca, cb))
    finally:
        on.close()
        off.close()
    assert set(cap) == set(ctx) | {"capture_clip_kernel"} and "capture_clip_kernel" not in ctx
    assert cap["capture_clip_kernel"] == 1 and cap["stft_context_features"] == 1 and ctx["stft_context_features"] == 2
    assert "cond_proj" not in cap and not [k for k in cap if k.startswith("online_")]
    for k in ctx:
        assert cap[k] <= ctx[k], k


def test_row_against_the_float64_oracle(eng, weights_denoiser):
    """Sanity in float64: the captured row against oracle.nhans_oracle.embed_tower on the same float32 features, within the
    bar tests/test_gpu_recipes.py holds tower rows to (EMB_TOL * max(1, max|row|)); no new number."""
    import oracle.nhans_oracle as O
    x = _x()
    enh = _open(eng, 1)
    try:
        _push_to(enh, x, [NTOT])
        enh.capture_context(0, "b", normalise=False)
        got = enh.embeddings(0)[1]
    finally:
        enh.close()
    feat = _features(eng, x[NTOT - CAP:]).cpu().numpy().astype(np.float64)
    ref = O.embed_tower(feat, weights_denoiser)[0]
    err = float(np.abs(got - ref).max())
    print("captured row against float64: max |d| = %.3e, max |row| = %.3e" % (err, float(np.abs(ref).max())))
    assert err <= EMB_TOL * max(1.0, float(np.abs(ref).max()))
