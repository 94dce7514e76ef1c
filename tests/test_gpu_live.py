"""Live PCM sessions on the device (nhans_live_*, n-hans_amd/live.py): device-rate pieces in, device-rate PCM out, bit
for bit the offline chain resample -> fixed peak -> trim -> enhance -> wet/dry mix -> resample -> scale -> round, for
seeded cuttings, a wet factor changed mid-stream, rewind and the saturation fallback, slots that join and are reused,
argument errors, the launch count of a push, and the torch-free engine."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, resample, spec, synth
# (no torch at import time: the torch-free worker below is unpickled from this module in a fresh process)

pytestmark = pytest.mark.gpu

PEAK = 21000
# (rate in, dtype in, rate out, dtype out): both converters carrying / the longest input table and the copy on output /
# the copy on input and the 16 -> 44.1 kHz table on output
CONFIGS = [(48000, np.int16, 48000, np.int16), (44100, np.float32, 16000, np.float32), (16000, np.int16, 44100, np.int16)]
CONFIG_IDS = ["48k_i16-48k_i16", "44k1_f32-16k_f32", "16k_i16-44k1_i16"]


def _engine(*args, **kw):
    from nhans_amd import engine
    return engine.Engine(*args, **kw)


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


def _recording(rate, seed, dtype=np.int16):
    """About 1.3 s (128 frames at 16 kHz) on the int16 scale at `rate`, with a tail that fills no hop."""
    base = synth.mixture(seed, 1.3)
    if rate == 48000:
        x = np.repeat(base, 3)[:-101]
    elif rate == 16000:
        x = base[:-57]
    else:
        n = int(len(base) * rate / 16000) - 37
        x = np.round(np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(base)), base.astype(np.float64)))
    return np.ascontiguousarray(x.astype(dtype))


def _ctx(seed):
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(seed))


_offline = {}


def _den_mix(e, rate, dtype, seed):
    """The offline 16 kHz results of recording (rate, seed): computed once, shared, never written to."""
    key = (rate, np.dtype(dtype).name, seed)
    if key not in _offline:
        y = resample.resample(e, [_recording(rate, seed, dtype)], rate, 16000)[0]
        m = apply.trim_to_frames(online.normalise_fixed(y, PEAK))
        ca, cb = _ctx(seed)
        r = e.enhance([m], [ca], [cb], want_mixed=True)
        den, mix = r["denoised_wav"][0], r["mixed_wav"][0]
        assert den.dtype == mix.dtype == np.float32 and len(den) == len(mix) == len(m) > 16000
        den.setflags(write=False); mix.setflags(write=False)
        _offline[key] = (den, mix)
    return _offline[key]


def _combine(den, mix, w):
    c = den + (mix - den) * np.float32(w)
    assert c.dtype == np.float32
    return c


def _converted(e, c, out_rate):
    return resample.resample(e, [c], 16000, out_rate)[0]


def _pcm(y, out_dtype, scale):
    v = (y.astype(np.float64) * scale).astype(np.float32)
    if np.dtype(out_dtype) == np.float32:
        return v
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def _cut(rng, n):
    out, left = [], n
    while left > 0:
        k = min(int(rng.choice([0, 1, 7, 160, 441, 480, 4800])), left)
        out.append(k)
        left -= k
    return out or [0]


def _even(n, k):
    return [min(k, n - a) for a in range(0, n, k)]


def _run(sess, plans, before_push=None):
    """plans[i]: the recordings slot i carries one after the other, each dict(x, cuts, join, ctx): the slot joins
    (restart + set_context(*ctx), ctx None: conditioned already) at the first step >= join at which it is free.  Every
    push's counts are checked against out_counts and live.emitted.  -> per slot, the concatenated output of each
    recording."""
    S = sess.S
    rates = (sess.in_rate, sess.out_rate)
    queue = [list(p) for p in plans]
    now = [None] * S
    outs = [[] for _ in range(S)]
    step = 0
    while any(queue) or any(n is not None for n in now):
        for i in range(S):
            if now[i] is None and queue[i] and step >= queue[i][0].get("join", 0):
                now[i] = dict(queue[i].pop(0), pos=0, k=0, got=[])
                sess.restart(i)
                if now[i].get("ctx") is not None:
                    sess.set_context(i, *now[i]["ctx"])
        chunks, end = [], []
        for i in range(S):
            r = now[i]
            if r is None:
                chunks.append(np.zeros(0, sess.in_dtype)); end.append(False)
                continue
            n = r["cuts"][r["k"]]
            r["k"] += 1
            chunks.append(r["x"][r["pos"]:r["pos"] + n])
            r["pos"] += n
            end.append(r["k"] == len(r["cuts"]))
        if before_push is not None:
            before_push(step, chunks, end)
        want = [live.emitted(sess.pushed[i] + len(chunks[i]), bool(end[i] or sess.ended[i]), *rates) -
                live.emitted(sess.pushed[i], sess.ended[i], *rates) for i in range(S)]
        assert sess.out_counts([len(c) for c in chunks], end) == want
        got = sess.push(chunks, end)
        for i in range(S):
            assert got[i].dtype == sess.out_dtype and len(got[i]) == want[i]
            if now[i] is not None:
                now[i]["got"].append(got[i])
                if end[i]:
                    assert now[i]["pos"] == len(now[i]["x"])
                    outs[i].append(np.concatenate(now[i]["got"]))
                    now[i] = None
            else:
                assert len(got[i]) == 0
        step += 1
    return outs


@pytest.mark.parametrize("wet", [0.0, 0.25])
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_bit_for_bit_the_offline_chain(eng, config, wet):
    """Three slots, each on its own seeded cutting of 0, 1, 7, 160, 441, 480 and 4,800-sample pushes.  int16 output:
    out_scale is twice what would put the smaller of the two extremes of the expected signal on its rail, so both rails
    clip and most samples do not."""
    rate_in, dt_in, rate_out, dt_out = config
    seeds = [911, 912, 913]
    ys = [_converted(eng, _combine(*_den_mix(eng, rate_in, dt_in, s), wet), rate_out) for s in seeds]
    if np.dtype(dt_out) == np.int16:
        scale = 2.0 * 32767.0 / min(min(float(y.max()), float(-y.min())) for y in ys)
    else:
        scale = 1.0
    want = [_pcm(y, dt_out, scale) for y in ys]
    if np.dtype(dt_out) == np.int16:
        for w in want:
            assert (w == 32767).any() and (w == -32768).any() and (np.abs(w.astype(np.int32)) < 20000).sum() > len(w) // 4
    rng = np.random.default_rng(300 + CONFIGS.index(config))
    xs = [_recording(rate_in, s, dt_in) for s in seeds]
    plans = [[dict(x=x, cuts=_cut(rng, len(x)), ctx=_ctx(s))] for x, s in zip(xs, seeds)]
    sess = live.LiveSession(eng, 3, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, out_scale=scale, wet=wet != 0)
    try:
        sess.set_wet(wet)
        outs = _run(sess, plans)
    finally:
        sess.close()
    for i in range(3):
        got, = outs[i]
        assert len(got) == len(want[i]) == live.emitted(len(xs[i]), True, rate_in, rate_out)
        assert got.dtype == want[i].dtype and np.array_equal(got, want[i]), (config, wet, i)


def test_equals_online_enhancer_where_they_overlap(eng):
    """float32 out, out_scale 1, wet 0, 48 kHz both ways, 10 ms pieces: the denoised output of OnlineEnhancer(in_rate,
    out_rate, peak), piece by piece."""
    x = _recording(48000, 911)
    ca, cb = _ctx(911)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, out_dtype=np.float32)
    enh = online.OnlineEnhancer(eng, [ca], [cb], in_rate=48000, out_rate=48000, peak=PEAK)
    try:
        assert sess.out_scale == 1.0
        sess.set_context(0, ca, cb)
        for a in range(0, len(x), 480):
            end = [a + 480 >= len(x)]
            got, = sess.push([x[a:a + 480]], end)
            (ref, _), = enh.push([x[a:a + 480]], end)
            assert got.dtype == np.float32 and np.array_equal(got, ref), a
    finally:
        sess.close()
        enh.close()


def test_wet_changes_mid_stream(eng):
    """set_wet(0.5) after the sixth push: the 16 kHz samples final before it (online.emitted of what the incoming
    converter had emitted) keep w = 0, the later ones get 0.5, and the output is the conversion of that piecewise c."""
    x = _recording(48000, 912)
    den, mix = _den_mix(eng, 48000, np.int16, 912)
    cuts = _even(len(x), 4800)
    n_before = sum(cuts[:6])
    split = online.emitted(resample.emitted(n_before, False, 48000, 16000), False)
    assert 0 < split < len(den)
    c = np.concatenate([den[:split], _combine(den, mix, 0.5)[split:]])
    scale = live.default_out_scale(PEAK, np.int16)
    want = _pcm(_converted(eng, c, 48000), np.int16, scale)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, wet=True)
    try:
        assert sess.out_scale == scale
        outs = _run(sess, [[dict(x=x, cuts=cuts, ctx=_ctx(912))]],
                    before_push=lambda step, chunks, end: sess.set_wet(0.5) if step == 6 else None)
    finally:
        sess.close()
    assert np.array_equal(outs[0][0], want)
    assert not np.array_equal(want, _pcm(_converted(eng, den, 48000), np.int16, scale))


def test_rewind(eng):
    """Push, rewind, push the same pieces: that push and every later one give what a run without the rewind gives;
    a second rewind, one before any push and one after restart / set_context are NHANS_EINVAL."""
    lib = hip.load()
    x = _recording(44100, 913, np.float32)
    ca, cb = _ctx(913)
    den, mix = _den_mix(eng, 44100, np.float32, 913)
    want = _pcm(_converted(eng, _combine(den, mix, 0.25), 44100), np.int16, 9000.0)
    cuts = _even(len(x), 4410)
    sess = live.LiveSession(eng, 1, 44100, 44100, PEAK, in_dtype=np.float32, out_scale=9000.0, wet=True)
    try:
        sess.set_wet(0.25)
        assert lib.nhans_live_rewind(sess.handle) == -1 and b"nhans_live_rewind" in lib.nhans_last_error()
        sess.set_context(0, ca, cb)
        outs, pos = [], 0
        for k, n in enumerate(cuts):
            piece, end = x[pos:pos + n], [k == len(cuts) - 1]
            got, = sess.push([piece], end)
            if k in (0, 7, 8, len(cuts) - 1):             # the first push, two that emit, the one that ends the stream
                sess.rewind()
                assert lib.nhans_live_rewind(sess.handle) == -1
                again, = sess.push([piece], end)
                assert np.array_equal(again, got), k
            outs.append(got)
            pos += n
        assert np.array_equal(np.concatenate(outs), want)
        with pytest.raises(hip.NhansError):
            sess.push([x[:10]])                           # (the stream has ended, also after the rewound end)
        sess.restart(0)
        assert lib.nhans_live_rewind(sess.handle) == -1
        sess.push([x[:4410]])
        sess.set_context(0, ca, cb)
        assert lib.nhans_live_rewind(sess.handle) == -1
        sess.push([x[4410:8820]])
        sess.rewind()
    finally:
        sess.close()


def test_rewind_where_the_stages_differ_per_slot(eng):
    """Three slots, 44.1 kHz float32 in, 48 kHz int16 out, wet 0.25.  The pushes that are rewound bring 0 samples to one
    slot, 1 to another and 4,410 to the third, the roles turning: the 1-sample slot's incoming converter flips its carried
    half while its outgoing one, which got nothing, does not, so the three stages' snapshots must each be the slot's own.
    The last push ends all three slots (with 4,410, 1 and 0 samples) and is rewound too.  The push after a rewind gives
    the same bytes, and every slot's stream is bit for bit its offline chain (the `want` of
    test_bit_for_bit_the_offline_chain)."""
    seeds = [911, 912, 913]
    xs = [_recording(44100, s, np.float32) for s in seeds]
    ys = [_converted(eng, _combine(*_den_mix(eng, 44100, np.float32, s), 0.25), 48000) for s in seeds]
    scale = 2.0 * 32767.0 / min(min(float(y.max()), float(-y.min())) for y in ys)
    want = [_pcm(y, np.int16, scale) for y in ys]
    roles, tail = [4410, 1, 0], [4410, 1, 0]
    left = [len(x) - t for x, t in zip(xs, tail)]         # what a slot brings before the last push
    steps = []                                            # (counts, end, rewound)
    while any(left):
        k = len(steps)
        counts = [roles[(i + k) % 3] for i in range(3)] if k in (0, 4, 8) else [4410] * 3
        counts = [min(c, l) for c, l in zip(counts, left)]
        assert k not in (0, 4, 8) or sorted(counts) == [0, 1, 4410]
        left = [l - c for l, c in zip(left, counts)]
        steps.append((counts, [False] * 3, k in (0, 4, 8)))
    assert len(steps) > 9
    steps.append((tail, [True] * 3, True))
    sess = live.LiveSession(eng, 3, 44100, 48000, PEAK, in_dtype=np.float32, out_scale=scale, wet=True)
    try:
        sess.set_wet(0.25)
        for i, s in enumerate(seeds):
            sess.set_context(i, *_ctx(s))
        outs, pos = [[] for _ in range(3)], [0, 0, 0]
        for k, (counts, end, rewound) in enumerate(steps):
            pieces = [x[p:p + n] for x, p, n in zip(xs, pos, counts)]
            got = sess.push(pieces, end)
            if rewound:
                sess.rewind()
                again = sess.push(pieces, end)
                for i in range(3):
                    assert again[i].tobytes() == got[i].tobytes(), (k, i)
            for i in range(3):
                outs[i].append(got[i])
                pos[i] += counts[i]
        assert pos == [len(x) for x in xs] and sess.ended == [True] * 3
    finally:
        sess.close()
    assert any(len(o) for o in outs[0][4:5] + outs[1][4:5] + outs[2][4:5])       # (the rewound pushes are not all silent)
    for i in range(3):
        got = np.concatenate(outs[i])
        assert got.dtype == np.int16 and len(got) == live.emitted(len(xs[i]), True, 44100, 48000)
        assert np.array_equal(got, want[i]), i


def _scaled_block1(weights_denoiser):           # (as tests/test_gpu_online.py)
    W = dict(weights_denoiser)
    W["resblock1_1_conv1/w"] = (W["resblock1_1_conv1/w"] * np.float32(3.0e5)).astype(np.float32)
    return W


def test_saturated_push_is_redone_in_f32(lib_built, weights_denoiser):
    """Exponents forced to zero on weights that overflow f16: the push warns and gives the bits of the same push made at
    precision f32 (a second session of the same engine: same conditioning, only the push at f32); the precision is
    restored and the exponents have risen."""
    W = _scaled_block1(weights_denoiser)
    x = _recording(48000, 911)[:48000 * 6 // 10]
    ca, cb = _ctx(911)

    def one_push(e, push_precision):
        sess = live.LiveSession(e, 1, 48000, 48000, PEAK, out_dtype=np.float32, wet=True)
        try:
            sess.set_context(0, ca, cb)
            sess.set_wet(0.25)
            e.set_precision(push_precision)
            return sess.push([x], end=[True])[0]
        finally:
            e.set_precision("f16x3")
            sess.close()

    e16 = _engine("denoiser", W, precision="f16x3")
    try:
        e16.set_activation_exponents([0] * hip.NUM_ACTIVATIONS)
        tower = e16.activation_exponents()[:8]
        with pytest.warns(UserWarning, match="f16 range"):
            got = one_push(e16, "f16x3")
        assert e16.precision == "f16x3" and max(e16.activation_exponents()) >= 10
        assert e16.activation_exponents()[:8] == tower        # (the push runs no tower: the conditioning below is the same)
        ref = one_push(e16, "f32")
    finally:
        e16.close()
    assert len(got) == live.emitted(len(x), True, 48000, 48000) > 0
    assert got.tobytes() == ref.tobytes()                 # (NaN where the scaled model overflows f32 too)


def test_slots_join_and_are_reused(eng):
    """Opened unconditioned: samples to such a slot are refused.  Slot 1 joins at step 9 with restart + set_context, is
    restarted after its recording has ended and carries a second one, while slots 0 and 2 run on; all four recordings
    are bit for bit their offline chains."""
    seeds = {0: [911], 1: [912, 913], 2: [914]}
    rng = np.random.default_rng(55)
    scale = live.default_out_scale(PEAK, np.int16)
    sess = live.LiveSession(eng, 3, 48000, 48000, PEAK)
    try:
        x = _recording(48000, 911)
        with pytest.raises(hip.NhansError, match="conditioning"):
            sess.push([x[:480], x[:0], x[:0]])
        with pytest.raises(hip.NhansError, match="conditioning"):
            sess.push([x[:0], x[:0], x[:0]], end=[False, True, False])
        assert [len(o) for o in sess.push([x[:0]] * 3)] == [0, 0, 0]
        plans = []
        for i in range(3):
            plans.append([])
            for k, s in enumerate(seeds[i]):
                r = _recording(48000, s)
                if i == 1:
                    r = r[:len(r) * 6 // 10]              # (two recordings pass through slot 1 while 0 and 2 carry one)
                cuts = _even(len(r), 480 * 5) if i != 1 else _cut(rng, len(r))
                plans[i].append(dict(x=r, cuts=cuts, join=9 if i == 1 else 0, ctx=_ctx(s)))
        outs = _run(sess, plans)
    finally:
        sess.close()
    for i in range(3):
        assert len(outs[i]) == len(seeds[i])
        for k, s in enumerate(seeds[i]):
            if i == 1:
                r = _recording(48000, s)
                r = r[:len(r) * 6 // 10]
                y = resample.resample(eng, [r], 48000, 16000)[0]
                m = apply.trim_to_frames(online.normalise_fixed(y, PEAK))
                den = eng.enhance([m], [_ctx(s)[0]], [_ctx(s)[1]], want_mixed=False)["denoised_wav"][0]
            else:
                den = _den_mix(eng, 48000, np.int16, s)[0]
            assert np.array_equal(outs[i][k], _pcm(_converted(eng, den, 48000), np.int16, scale)), (i, k)


def test_errors_change_nothing(eng):
    """Every refused call of the header's list between the pushes of a running stream: NHANS_EINVAL with the function's
    name, and the stream's output stays bit for bit the offline chain."""
    import torch
    lib = hip.load()
    i64 = hip.i64_array
    x = _recording(48000, 911)
    ca, cb = _ctx(911)
    scale = live.default_out_scale(PEAK, np.int16)
    want = _pcm(_converted(eng, _den_mix(eng, 48000, np.int16, 911)[0], 48000), np.int16, scale)
    h = ctypes.c_void_p()
    assert lib.nhans_live_open_slots(eng.handle, 3, 44000, 0, 1.0, 48000, 0, 1.0, 0, eng._stream(), ctypes.byref(h)) == -1
    assert b"44000" in lib.nhans_last_error() and b"48000" in lib.nhans_last_error() and b"nhans_live_open_slots" in lib.nhans_last_error()
    for args in ((0, 48000, 0, 1.0, 48000, 0, 1.0, 0), (3, 48000, 7, 1.0, 48000, 0, 1.0, 0), (3, 48000, 0, 1.0, 48000, 7, 1.0, 0),
                 (3, 48000, 0, -1.0, 48000, 0, 1.0, 0), (3, 48000, 0, 1.0, 48000, 0, 0.0, 0),
                 (3, 48000, 0, 1.0, 48000, 0, float("inf"), 0), (3, 48000, 0, 1.0, 48000, 0, 1.0, 2)):
        assert lib.nhans_live_open_slots(eng.handle, *args, eng._stream(), ctypes.byref(h)) == -1, args
        assert b"nhans_live_open_slots" in lib.nhans_last_error() and not h.value
    # slot 0 runs, slot 1 stays unconditioned, slot 2 is conditioned and ends at once
    sess = live.LiveSession(eng, 3, 48000, 48000, PEAK)
    din = torch.from_numpy(x).to(eng.device)
    dca, dcb = torch.from_numpy(ca).to(eng.device), torch.from_numpy(cb).to(eng.device)
    dout = torch.zeros(32768, dtype=torch.int16, device=eng.device)
    got = (ctypes.c_int64 * 3)()
    st = eng._stream()

    def push(ioff, end, ooff, in_ptr=hip.ptr(din), out_ptr=hip.ptr(dout)):
        return lib.nhans_live_push(sess.handle, in_ptr, i64(ioff) if ioff else None, (ctypes.c_int * 3)(*end) if end else None,
                                   out_ptr, i64(ooff) if ooff else None, got, st)

    def refused(rc, name):
        assert rc == -1 and name in lib.nhans_last_error(), (rc, lib.nhans_last_error())

    room = [0, 32768, 32768, 32768]
    bad = [
        lambda a, b: refused(push([a, b, b + 5, b + 5], None, room), b"conditioning"),                # unconditioned slot
        lambda a, b: refused(push([a, b, b, b], [0, 1, 0], room), b"nhans_live_push"),                # ... and its end
        lambda a, b: refused(push([a, b, b, b + 5], None, room), b"ended"),                           # ended slot
        lambda a, b: refused(push([a, b, b, b], [0, 0, 1], room), b"nhans_live_push"),
        lambda a, b: refused(push([b, a, a, a], None, room), b"nhans_live_push"),                     # negative count
        lambda a, b: refused(push([a, b, b, b], None, [0, 100, 100, 100]), b"room"),                  # too little room
        lambda a, b: refused(push([a, b, b, b], None, room, in_ptr=None), b"nhans_live_push"),        # NULLs
        lambda a, b: refused(push([a, b, b, b], None, room, out_ptr=None), b"nhans_live_push"),
        lambda a, b: refused(push(None, None, room), b"nhans_live_push"),
        lambda a, b: refused(push([a, b, b, b], None, None), b"nhans_live_push"),
        lambda a, b: refused(lib.nhans_live_restart(sess.handle, 3), b"nhans_live_restart"),          # slot out of range
        lambda a, b: refused(lib.nhans_live_restart(sess.handle, -1), b"nhans_live_restart"),
        lambda a, b: refused(lib.nhans_live_set_context(sess.handle, 3, hip.ptr(dca), len(ca), hip.ptr(dcb), len(cb), st, None),
                             b"nhans_live_set_context"),
        lambda a, b: refused(lib.nhans_live_set_context(sess.handle, 0, None, len(ca), hip.ptr(dcb), len(cb), st, None),
                             b"nhans_live_set_context"),
        lambda a, b: refused(lib.nhans_live_set_embeddings(sess.handle, 5, hip.ptr(dca), hip.ptr(dcb), st, None),
                             b"nhans_live_set_embeddings"),
        lambda a, b: refused(lib.nhans_live_set_embeddings(sess.handle, 0, None, hip.ptr(dcb), st, None),
                             b"nhans_live_set_embeddings"),
        lambda a, b: refused(lib.nhans_live_set_wet(sess.handle, 0.3), b"NHANS_LIVE_WET"),            # opened without the flag
        lambda a, b: refused(lib.nhans_live_set_wet(sess.handle, float("nan")), b"nhans_live_set_wet"),
        lambda a, b: refused(lib.nhans_live_out_counts(sess.handle, i64([-1, 0, 0]), None, got), b"nhans_live_out_counts"),
    ]
    try:
        sess.set_context(0, ca, cb)
        sess.set_context(2, ca, cb)
        assert lib.nhans_live_set_wet(sess.handle, 0.0) == 0
        assert push([0, 0, 0, 0], [0, 0, 1], room) == 0 and list(got) == [0, 0, 0]
        outs, k = [], 0
        for a in range(0, len(x), 4800):
            b = min(a + 4800, len(x))
            for _ in range(2):
                bad[k % len(bad)](a, b)
                k += 1
            assert push([a, b, b, b], [int(b == len(x)), 0, 0], room) == 0
            assert got[1] == got[2] == 0
            outs.append(dout[:got[0]].cpu().numpy())
        assert k >= len(bad)
    finally:
        sess.close()
    assert np.array_equal(np.concatenate(outs), want)


def test_one_call_and_no_detour(eng):
    """A steady-state push is one live_in launch, at most one live_out launch and none of the stand-alone converters';
    the device-tensor variant takes and returns tensors on the engine's device, with the bits of the chain."""
    import torch
    x = _recording(48000, 911)
    scale = live.default_out_scale(PEAK, np.int16)
    want = _pcm(_converted(eng, _den_mix(eng, 48000, np.int16, 911)[0], 48000), np.int16, scale)
    din = torch.from_numpy(x).to(eng.device)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK)
    outs, launches = [], []
    try:
        sess.set_context(0, *_ctx(911))
        for a in range(0, len(x), 480):
            b = min(a + 480, len(x))
            steady = 60 <= a // 480 < 70
            if steady:
                eng.set_option("profile", 1)
                eng.profile_reset()
            try:
                out, off = sess.push_device(din[a:b], [b - a], end=[b == len(x)])
                if steady:
                    launches.append(eng.profile())
            finally:
                if steady:
                    eng.set_option("profile", 0)
            assert out.device == torch.device(eng.device) and out.dtype == torch.int16 and off == [0, out.numel()]
            outs.append(out)
    finally:
        sess.close()
    assert np.array_equal(torch.cat(outs).cpu().numpy(), want)
    assert len(launches) == 10
    for prof in launches:
        assert prof["live_in"]["calls"] == 1
        assert prof.get("live_out", {"calls": 0})["calls"] <= 1
        assert "resampler_push" not in prof and "resample" not in prof
    assert sum(prof.get("live_out", {"calls": 0})["calls"] for prof in launches) >= 4      # (every second hop emits)


def _live_48k(e):
    x = _recording(48000, 911)
    rng = np.random.default_rng(8)
    sess = live.LiveSession(e, 1, 48000, 48000, PEAK, wet=True)
    try:
        sess.set_wet(0.25)
        return _run(sess, [[dict(x=x, cuts=_cut(rng, len(x)), ctx=_ctx(911))]])[0][0]
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
        out = _live_48k(le)
        le.close()
        q.put((out, "torch" in sys.modules, None))
    except Exception as e:
        import traceback
        q.put((None, None, traceback.format_exc() + repr(e)))


def test_live_48k_over_the_torch_free_engine(eng):
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_lite_worker, args=(q,))
    p.start()
    try:
        out, had_torch, err = q.get(timeout=600)
    finally:
        p.join(timeout=120)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert had_torch is False
    assert out.dtype == np.int16 and np.array_equal(out, _live_48k(eng))
    den, mix = _den_mix(eng, 48000, np.int16, 911)
    assert np.array_equal(out, _pcm(_converted(eng, _combine(den, mix, 0.25), 48000), np.int16, live.default_out_scale(PEAK, np.int16)))
