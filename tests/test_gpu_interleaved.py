"""Live sessions on interleaved frames (nhans_interleaved_*, live.LiveSession(channels=...)): every output is compared BIT
FOR BIT with a mono LiveSession of the same engine, rates, peak, look-ahead and conditioning doing the same pushes -- the
downmix against a mono float32 slot fed live.downmix(frames), a split stream against one mono slot per channel -- for
seeded cuttings, the wet factor fixed, changed and automatic, rewind and the saturation fallback, capture, the launches of
a push, and the refusals."""
import ctypes

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, context, hip, live, synth

pytestmark = pytest.mark.gpu

PEAK = 21000
# (as tests/test_gpu_live.py) both converters carrying / the longest input table and the copy on output / the copy on input
# and the 16 -> 44.1 kHz table on output
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


def _recording(rate, seed, dtype=np.int16, seconds=1.3):
    """(tests/test_gpu_live.py) about 1.3 s on the int16 scale at `rate`, with a tail that fills no hop."""
    base = synth.mixture(seed, seconds)
    if rate == 48000:
        x = np.repeat(base, 3)[:-101]
    elif rate == 16000:
        x = base[:-57]
    else:
        n = int(len(base) * rate / 16000) - 37
        x = np.round(np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(base)), base.astype(np.float64)))
    return np.ascontiguousarray(x.astype(dtype))


_frames = {}


def _interleaved(rate, seeds, dtype, drop=0, seconds=1.3):
    """[n, len(seeds)] frames, channel c the recording of seeds[c] (`drop` frames shorter); float32 channels are scaled by
    factors that are no powers of two, so that their values are no integers and the order and width of the sum show.
    Made once, shared, never written to."""
    key = (rate, tuple(seeds), np.dtype(dtype).name, drop, seconds)
    if key not in _frames:
        chans = [_recording(rate, s, dtype, seconds) for s in seeds]
        n = min(len(c) for c in chans) - drop
        x = np.stack([c[:n] for c in chans], axis=1)
        if np.dtype(dtype) == np.float32:
            x = x * np.array([0.37, 0.61, 0.83, 0.29][:len(seeds)], dtype=np.float32)
        x = np.ascontiguousarray(x.astype(dtype))
        x.setflags(write=False)
        _frames[key] = x
    return _frames[key]


def _ctx(seed):
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(seed))


def _cut(rng, n, big=0):
    """Pushes of 1, 7, 160, 441, 480 and 4,800 frames, 1-frame pushes (the carry alone) as the second and the fourth and,
    with `big`, one push of that many frames as the third."""
    out, left = [], n
    while left > 0:
        k = int(rng.choice([1, 7, 160, 441, 480, 4800, 4800]))
        if len(out) in (1, 3):
            k = 1
        if big and len(out) == 2:
            k = big
        k = min(k, left)
        out.append(k)
        left -= k
    assert not big or big in out
    return out


def _even(n, k):
    return [min(k, n - a) for a in range(0, n, k)]


def _drive(sess, xs, cuts, before_push=None, after_push=None, rewind_at=()):
    """xs[i] / cuts[i]: what slot (mono session) or stream (interleaved session) i is pushed, piece by piece, the last
    piece with its end flag; a finished one gets empty pieces.  -> per slot or stream its concatenated output."""
    n = len(xs)
    pos, k, outs = [0] * n, [0] * n, [[] for _ in range(n)]
    step = 0
    while any(k[i] < len(cuts[i]) for i in range(n)):
        chunks, end = [], []
        for i in range(n):
            m = cuts[i][k[i]] if k[i] < len(cuts[i]) else 0
            chunks.append(xs[i][pos[i]:pos[i] + m])
            pos[i] += m
            k[i] += 1
            end.append(k[i] == len(cuts[i]))
        if before_push is not None:
            before_push(step)
        want = sess.out_counts([len(c) for c in chunks], end)
        got = sess.push(chunks, end)
        if step in rewind_at:
            sess.rewind()
            again = sess.push(chunks, end)
            for i in range(n):
                assert again[i].tobytes() == got[i].tobytes(), (step, i)
        for i in range(n):
            assert got[i].dtype == sess.out_dtype and len(got[i]) == want[i]
            outs[i].append(got[i])
        if after_push is not None:
            after_push(step)
        step += 1
    assert pos == [len(x) for x in xs]
    return [np.concatenate(o) for o in outs]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- 1. downmix
@pytest.mark.parametrize("config", CONFIGS[:2], ids=CONFIG_IDS[:2])
def test_downmix_in_duplicate_out(eng, config):
    """Three channels in -- the division by 3 is inexact, which a float32 sum or a hard-coded 2 would show --, two out.
    Every output channel is the output of a mono float32-in slot fed live.downmix(frames), under one seeded cutting with
    1-frame pushes and one push of 9,611 frames (several runs of 1,024 outputs in both converters)."""
    rate_in, dt_in, rate_out, dt_out = config
    x = _interleaved(rate_in, (911, 912, 913), dt_in)
    mono_in = live.downmix(x)
    assert mono_in.dtype == np.float32
    cuts = _cut(np.random.default_rng(700 + CONFIGS.index(config)), len(x), big=9611)
    assert cuts.count(1) >= 2 and max(cuts) == 9611
    ref_sess = live.LiveSession(eng, 1, rate_in, rate_out, PEAK, in_dtype=np.float32, out_dtype=dt_out, out_scale=9000.0)
    sess = live.LiveSession(eng, 1, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, out_scale=9000.0, channels=3,
                            out_channels=2)
    try:
        assert sess.S == 1 and sess.slots_of(0) == [0]
        for s in (ref_sess, sess):
            s.set_context(0, *_ctx(911))
        ref, = _drive(ref_sess, [mono_in], [cuts])
        got, = _drive(sess, [x], [cuts])
    finally:
        sess.close()
        ref_sess.close()
    assert len(ref) == live.emitted(len(x), True, rate_in, rate_out) > rate_out
    assert got.shape == (len(ref), 2) and np.abs(ref.astype(np.float64)).max() > 0
    for c in range(2):
        assert _same(np.ascontiguousarray(got[:, c]), ref), c


# ---------------------------------------------------------------------------------------------- 2. split
def _raw_push(eng, sess, x, foff, end, out_dev, ooff):
    """nhans_interleaved_live_push on frames x (host, [n, C]) with caller-made frame offsets into out_dev."""
    import torch
    din = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(eng.device) if x.size else None
    got = (ctypes.c_int64 * sess.nstreams)()
    rc = sess.lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), hip.i64_array(foff), context.end_flags(end, sess.nstreams),
                                              hip.ptr(out_dev), hip.i64_array(ooff), got, eng._stream())
    return rc, list(got)


@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_split_equals_one_mono_slot_per_channel(eng, config):
    """Two stereo streams of different lengths in one object, each on its own cutting, a different context per channel:
    channel c of stream g is the mono session's slot 2 g + c fed that channel alone.  The output buffer is a sentinel
    with 5 spare frames of room after every stream: nothing outside a stream's frames is written."""
    import torch
    rate_in, dt_in, rate_out, dt_out = config
    xs = [_interleaved(rate_in, (911, 912), dt_in), _interleaved(rate_in, (913, 914), dt_in, drop=1234)]
    rng = np.random.default_rng(720 + CONFIGS.index(config))
    cuts = [_cut(rng, len(xs[0]), big=9611), _cut(rng, len(xs[1]))]
    seeds = [911, 912, 913, 914]
    ref_sess = live.LiveSession(eng, 4, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, out_scale=9000.0)
    sess = live.LiveSession(eng, 2, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, out_scale=9000.0, channels=2,
                            channel_mode="split")
    sentinel = -12345
    try:
        assert sess.S == 4 and sess.slots_of(0) == [0, 1] and sess.slots_of(1) == [2, 3]
        for s in (ref_sess, sess):
            for i, seed in enumerate(seeds):
                s.set_context(i, *_ctx(seed))
        ref = _drive(ref_sess, [np.ascontiguousarray(xs[i // 2][:, i % 2]) for i in range(4)], [cuts[i // 2] for i in range(4)])
        outs, pos = [[], []], [0, 0]
        for k in range(max(len(c) for c in cuts)):
            n = [cuts[g][k] if k < len(cuts[g]) else 0 for g in range(2)]
            end = [k == len(cuts[g]) - 1 for g in range(2)]
            x = np.concatenate([xs[g][pos[g]:pos[g] + n[g]] for g in range(2)])
            need = sess.out_counts(n, end)
            ooff = [0, need[0] + 5, need[0] + need[1] + 10]
            out_dev = torch.full((2 * ooff[2] + 8,), sentinel, dtype=getattr(torch, np.dtype(dt_out).name), device=eng.device)
            rc, got = _raw_push(eng, sess, x, [0, n[0], n[0] + n[1]], end, out_dev, ooff)
            assert rc == 0 and got == need, (k, sess.lib.nhans_last_error())
            out = out_dev.cpu().numpy()
            written = np.zeros(len(out), dtype=bool)
            for g in range(2):
                written[2 * ooff[g]:2 * (ooff[g] + got[g])] = True
                outs[g].append(out[2 * ooff[g]:2 * (ooff[g] + got[g])].reshape(-1, 2))
                pos[g] += n[g]
            assert (out[~written] == sentinel).all(), k
    finally:
        sess.close()
        ref_sess.close()
    for g in range(2):
        got = np.concatenate(outs[g])
        assert len(got) == live.emitted(len(xs[g]), True, rate_in, rate_out)
        for c in range(2):
            assert _same(np.ascontiguousarray(got[:, c]), ref[2 * g + c]), (g, c)
    assert not _same(ref[0], ref[1])


# ---------------------------------------------------------------------------------------------- 3. the outgoing mix policies
@pytest.mark.parametrize("dt_out", [np.int16, np.float32], ids=["i16", "f32"])
def test_split_with_the_fixed_and_the_automatic_mix(eng, dt_out):
    """wet 0.3 (no power of two) from the start, 0.7 from push 6, the meter and the automatic factor over 8 hops from
    push 12: the fixed and the automatic mix source in front of the interleaved sink.  Output, last_gains and levels of
    every slot are the mono session's, push by push."""
    x = _interleaved(48000, (911, 912), np.int16)
    cuts = _even(len(x), 2400)
    assert len(cuts) > 20
    seen = {}

    def hooks(s, tag):
        def before(step):
            if step == 0:
                s.set_wet(0.3)
            if step == 6:
                s.set_wet(0.7)
            if step == 12:
                s.enable_levels()
                s.set_auto_wet(window_hops=8)

        def after(step):
            if step >= 12:
                for i in range(2):
                    g = s.last_gains(i)
                    lv = s.levels(i) if len(g) else None
                    seen.setdefault(tag, []).append((step, i, g.tobytes(), repr(lv)))
        return before, after

    ref_sess = live.LiveSession(eng, 2, 48000, 48000, PEAK, out_dtype=dt_out, wet=True)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, out_dtype=dt_out, wet=True, channels=2, channel_mode="split")
    try:
        for s in (ref_sess, sess):
            s.set_context(0, *_ctx(911))
            s.set_context(1, *_ctx(912))
        ref = _drive(ref_sess, [np.ascontiguousarray(x[:, c]) for c in range(2)], [cuts, cuts], *hooks(ref_sess, "mono"))
        got, = _drive(sess, [x], [cuts], *hooks(sess, "frames"))
    finally:
        sess.close()
        ref_sess.close()
    for c in range(2):
        assert _same(np.ascontiguousarray(got[:, c]), ref[c]), c
    assert seen["frames"] == seen["mono"]
    gains = [b"".join(g for _, i, g, _ in seen["mono"] if i == c) for c in range(2)]
    assert len(gains[0]) == len(gains[1]) > 4 * 30 and gains[0] != gains[1]      # (per slot: the channels' factors differ)


# ---------------------------------------------------------------------------------------------- 4. rewind and redo
def test_rewind_and_redo(eng):
    """Pushes 0, 7, 8 and the last one are rewound and made again: the same bytes, and the concatenated output is the
    mono session's uninterrupted run -- a downmix stream and, in a second object, a split one."""
    x = _interleaved(44100, (911, 912), np.float32)
    cuts = _even(len(x), 4410)
    at = (0, 7, 8, len(cuts) - 1)
    kw = dict(in_dtype=np.float32, out_scale=9000.0, wet=True)
    ref_sess = live.LiveSession(eng, 3, 44100, 48000, PEAK, **kw)
    down = live.LiveSession(eng, 1, 44100, 48000, PEAK, channels=2, out_channels=1, **kw)
    split = live.LiveSession(eng, 1, 44100, 48000, PEAK, channels=2, channel_mode="split", **kw)
    try:
        for s in (ref_sess, down, split):
            s.set_wet(0.25)
            for i in range(s.S):
                s.set_context(i, *_ctx(911 + i % 2))
        ref = _drive(ref_sess, [np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1]), live.downmix(x)], [cuts] * 3)
        got_split, = _drive(split, [x], [cuts], rewind_at=at)
        got_down, = _drive(down, [x], [cuts], rewind_at=at)
    finally:
        for s in (ref_sess, down, split):
            s.close()
    assert got_down.shape == (len(ref[2]), 1) and _same(np.ascontiguousarray(got_down[:, 0]), ref[2])
    for c in range(2):
        assert _same(np.ascontiguousarray(got_split[:, c]), ref[c]), c


def test_saturated_push_is_redone_in_f32(lib_built, weights_denoiser):
    """(tests/test_gpu_live.py) exponents forced to zero on weights that overflow f16: the interleaved push warns, is
    rewound and redone, and gives the bits of the mono session's push made at precision f32."""
    W = dict(weights_denoiser)
    W["resblock1_1_conv1/w"] = (W["resblock1_1_conv1/w"] * np.float32(3.0e5)).astype(np.float32)
    x = _interleaved(48000, (911, 912), np.int16)[:48000 * 6 // 10]
    ca, cb = _ctx(911)

    def one_push(e, precision, **kw):
        sess = live.LiveSession(e, 2 if not kw else 1, 48000, 48000, PEAK, out_dtype=np.float32, wet=True, **kw)
        try:
            for i in range(2):
                sess.set_context(i, ca, cb)
            sess.set_wet(0.25)
            e.set_precision(precision)
            return sess.push([x] if kw else [np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1])], end=[True] * (1 if kw else 2))
        finally:
            e.set_precision("f16x3")
            sess.close()

    e16 = _engine("denoiser", W, precision="f16x3")
    try:
        e16.set_activation_exponents([0] * hip.NUM_ACTIVATIONS)
        with pytest.warns(UserWarning, match="f16 range"):
            got, = one_push(e16, "f16x3", channels=2, channel_mode="split")
        assert e16.precision == "f16x3" and max(e16.activation_exponents()) >= 10
        ref = one_push(e16, "f32")
    finally:
        e16.close()
    assert got.shape == (live.emitted(len(x), True, 48000, 48000), 2)
    for c in range(2):
        assert np.ascontiguousarray(got[:, c]).tobytes() == ref[c].tobytes()      # (NaN where the scaled model overflows f32 too)


# ---------------------------------------------------------------------------------------------- 5. capture
def test_capture_on_one_channel_of_a_split_stream(eng):
    """capture_context on the slot of channel 1 stores the row the mono session's slot 1 stores, and leaves channel 0's
    rows alone.  (The captured span is 2.015 s of 16 kHz samples, so this recording is 2.2 s -- in four pushes.)"""
    x = _interleaved(48000, (943, 944), np.int16, seconds=2.2)
    cuts = [4801, 1, 60000 - 4802, len(x) - 60000]
    ref_sess = live.LiveSession(eng, 2, 48000, 48000, PEAK)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, channels=2, channel_mode="split")
    rows = {}
    try:
        for tag, s in (("mono", ref_sess), ("frames", sess)):
            for i in range(2):
                s.set_context(i, *_ctx(911 + i))
            s.enable_capture()
            pos = 0
            for n in cuts:
                piece = x[pos:pos + n]
                s.push([piece] if s is sess else [np.ascontiguousarray(piece[:, 0]), np.ascontiguousarray(piece[:, 1])])
                pos += n
            before = s.embeddings(0) + s.embeddings(1)
            R = s.capture_contexts([(s.slots_of(0)[1] if s is sess else 1, "neg")], normalise=True)
            rows[tag] = (R, before, s.embeddings(0), s.embeddings(1))
    finally:
        sess.close()
        ref_sess.close()
    (R, before, e0, e1), (Rm, before_m, m0, m1) = rows["frames"], rows["mono"]
    assert R == Rm and R[0] > 0
    for a, b in zip(before + e0 + e1, before_m + m0 + m1):
        assert _same(a, b)
    assert all(_same(a, b) for a, b in zip(before[:3], e0 + e1[:1]))         # (channel 0's rows and channel 1's side a stay)
    assert not _same(e1[1], before[3])                                        # (side b of channel 1 is a new row)


# ---------------------------------------------------------------------------------------------- 6. launches
def _calls(e, fn):
    e.set_option("profile", 1)
    e.profile_reset()
    try:
        fn()
        return {k: v["calls"] for k, v in e.profile().items() if v["calls"]}
    finally:
        e.set_option("profile", 0)


@pytest.mark.parametrize("mode", ["downmix", "split"])
def test_a_push_issues_the_launches_of_a_mono_object(eng, mode):
    """Kernel names and counts of one steady-state push (4,800 frames, the meter on): identical for the interleaved object
    and for a mono object of the same slot count and piece sizes -- no de-interleave launch, no copy."""
    x = _interleaved(48000, (911, 912), np.int16)
    S = 2 if mode == "split" else 1
    ref_sess = live.LiveSession(eng, S, 48000, 48000, PEAK, wet=True)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, wet=True, channels=2, channel_mode=mode)
    calls = {}
    try:
        for tag, s in (("mono", ref_sess), ("frames", sess)):
            for i in range(S):
                s.set_context(i, *_ctx(911))
            s.set_wet(0.3)
            s.enable_levels()
            for k in range(6):
                piece = x[4800 * k:4800 * (k + 1)]
                chunks = [piece] if s is sess else [np.ascontiguousarray(piece[:, c]) for c in range(S)]
                if k < 5:
                    s.push(chunks)
                else:
                    calls[tag] = _calls(eng, lambda: s.push(chunks))
    finally:
        sess.close()
        ref_sess.close()
    assert calls["frames"] == calls["mono"]
    assert calls["mono"]["live_in"] == calls["mono"]["live_out"] == calls["mono"]["live_level"] == 1
    assert "channel_mean" not in calls["frames"] and "resample" not in calls["frames"]


def test_push_device_takes_and_returns_the_flat_frames(eng):
    """push_device on the flat interleaved tensor, counts and offsets in frames: the bytes push returns from a twin
    object, for a downmix (2 channels in, 3 out) and a split stream, and tensors on the engine's device both ways."""
    import torch
    x = _interleaved(48000, (911, 912), np.int16)
    cuts = _even(len(x), 4800)
    din = torch.from_numpy(np.array(x).reshape(-1)).to(eng.device)
    for kw, co in ((dict(channels=2, out_channels=3), 3), (dict(channels=2, channel_mode="split"), 2)):
        a = live.LiveSession(eng, 1, 48000, 48000, PEAK, **kw)
        b = live.LiveSession(eng, 1, 48000, 48000, PEAK, **kw)
        try:
            for s in (a, b):
                for i in range(s.S):
                    s.set_context(i, *_ctx(911 + i))
            pos = 0
            for k, n in enumerate(cuts):
                end = [k == len(cuts) - 1]
                want, = a.push([x[pos:pos + n]], end)
                out, off = b.push_device(din[2 * pos:2 * (pos + n)], [n], end)
                assert out.device == torch.device(eng.device) and out.dtype == torch.int16
                assert off == [0, len(want)] and out.numel() == co * len(want)
                assert _same(out.cpu().numpy().reshape(-1, co), want), (kw, k)
                pos += n
        finally:
            a.close()
            b.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing_and_launch_nothing(eng):
    """Every refusal of the header's list, made between the pushes of a running split stream with the profiler on: each
    is NHANS_EINVAL with its function's name, none issues a launch, and the stream's output stays the mono session's.
    One slot of the stream restarted alone: the push and the counts are refused, naming the stream and the slot, until
    the other slot is restarted too -- then both carry the recording again from its start."""
    import torch
    lib = hip.load()
    i64 = hip.i64_array
    x = _interleaved(48000, (911, 912), np.int16)
    cuts = _even(len(x), 4800)
    st = eng._stream()
    h = ctypes.c_void_p()

    def refused(rc, *words):
        msg = lib.nhans_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    def opened(nstreams, ci, co, mode):
        return lib.nhans_interleaved_live_open(eng.handle, nstreams, ci, co, mode, 48000, 0, 1.0, 48000, 0, 1.0, 0, st, ctypes.byref(h))

    ref_sess = live.LiveSession(eng, 2, 48000, 48000, PEAK)
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, channels=2, channel_mode="split")
    din = torch.from_numpy(np.array(x).reshape(-1)).to(eng.device)
    dout = torch.zeros(4 * 32768, dtype=torch.int16, device=eng.device)
    got = (ctypes.c_int64 * 2)()

    short = []

    def bad_calls(a, b):
        need = sess.out_counts([b - a])[0]
        for ci, co, mode in ((0, 2, 0), (9, 2, 0), (2, 0, 0), (2, 9, 0), (0, 0, 1), (9, 9, 1)):
            refused(opened(1, ci, co, mode), b"nhans_interleaved_live_open", b"channels")
            assert not h.value
        refused(opened(1, 2, 3, hip.INTERLEAVED_SPLIT), b"nhans_interleaved_live_open", b"NHANS_INTERLEAVED_SPLIT")
        refused(opened(1, 2, 2, 2), b"nhans_interleaved_live_open", b"mode")
        refused(opened(1, 2, 2, -1), b"nhans_interleaved_live_open", b"mode")
        refused(opened(0, 2, 2, 0), b"nhans_interleaved_live_open", b"nstreams")
        refused(lib.nhans_interleaved_live_open(eng.handle, 1, 2, 2, 0, 44000, 0, 1.0, 48000, 0, 1.0, 0, st, ctypes.byref(h)),
                b"nhans_interleaved_live_open", b"44000")
        refused(lib.nhans_interleaved_live_open(eng.handle, 1, 2, 2, 0, 48000, 7, 1.0, 48000, 0, 1.0, 0, st, ctypes.byref(h)),
                b"nhans_interleaved_live_open", b"in_format")
        assert not h.value
        # the mono pair on the interleaved object, the interleaved pair on the mono object
        refused(lib.nhans_live_push(sess.handle, hip.ptr(din), i64([a, b, b]), None, hip.ptr(dout), i64([0, 32768, 65536]), got, st),
                b"nhans_live_push", b"nhans_interleaved_live_push")
        refused(lib.nhans_live_out_counts(sess.handle, i64([b - a, b - a]), None, got), b"nhans_live_out_counts",
                b"nhans_interleaved_live_out_counts")
        refused(lib.nhans_interleaved_live_push(ref_sess.handle, hip.ptr(din), i64([a, b]), None, hip.ptr(dout), i64([0, 32768]), got, st),
                b"nhans_interleaved_live_push", b"nhans_live_push")
        refused(lib.nhans_interleaved_live_out_counts(ref_sess.handle, i64([b - a]), None, got), b"nhans_interleaved_live_out_counts",
                b"nhans_live_out_counts")
        # room one frame short; a negative count; NULLs
        if need > 0:
            short.append(need)
            refused(lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), i64([a, b]), None, hip.ptr(dout), i64([0, need - 1]), got, st),
                    b"nhans_interleaved_live_push", b"room", b"stream 0", b"frames")
            refused(lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), i64([a, b]), None, None, i64([0, need]), got, st),
                    b"nhans_interleaved_live_push")
        refused(lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), i64([b, a]), None, hip.ptr(dout), i64([0, 32768]), got, st),
                b"nhans_interleaved_live_push")
        refused(lib.nhans_interleaved_live_push(sess.handle, None, i64([a, b]), None, hip.ptr(dout), i64([0, 32768]), got, st),
                b"nhans_interleaved_live_push")
        refused(lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), None, None, hip.ptr(dout), i64([0, 32768]), got, st),
                b"nhans_interleaved_live_push")

    def out_of_step(a, b):
        refused(lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), i64([a, b]), None, hip.ptr(dout), i64([0, 32768]), got, st),
                b"nhans_interleaved_live_push", b"stream 0", b"slot 1", b"samples taken")
        refused(lib.nhans_interleaved_live_out_counts(sess.handle, i64([b - a]), None, got), b"nhans_interleaved_live_out_counts",
                b"stream 0", b"slot 1")
        refused(lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), i64([a, a]), (ctypes.c_int * 1)(1), hip.ptr(dout),
                                                i64([0, 32768]), got, st), b"nhans_interleaved_live_push", b"slot 1")

    def run(restart_after):
        """the recording's first restart_after pieces, then -- both slots restarted -- all of it"""
        outs_f, outs_m, pos = [], [], 0
        plan = cuts[:restart_after] + [None] + cuts
        for k, n in enumerate(plan):
            if n is None:
                eng.set_option("profile", 1)
                eng.profile_reset()
                try:
                    sess.restart(0)
                    out_of_step(pos, pos + 4800)
                    assert not any(v["calls"] for v in eng.profile().values())
                finally:
                    eng.set_option("profile", 0)
                # (a push that brings the stream neither frames nor its end moves no slot: it is taken)
                assert lib.nhans_interleaved_live_push(sess.handle, hip.ptr(din), i64([pos, pos]), None, hip.ptr(dout), i64([0, 0]), got, st) == 0
                assert got[0] == 0
                sess.restart(1)
                ref_sess.restart(0); ref_sess.restart(1)
                outs_f.append(None); outs_m.append(None)
                pos = 0
                continue
            eng.set_option("profile", 1)
            eng.profile_reset()
            try:
                bad_calls(pos, pos + n)
                assert not any(v["calls"] for v in eng.profile().values()), eng.profile()
            finally:
                eng.set_option("profile", 0)
            piece = x[pos:pos + n]
            end = k == len(plan) - 1
            outs_f.append(sess.push([piece], [end])[0])
            outs_m.append(ref_sess.push([np.ascontiguousarray(piece[:, 0]), np.ascontiguousarray(piece[:, 1])], [end] * 2))
            pos += n
        return outs_f, outs_m

    try:
        for s in (ref_sess, sess):
            s.set_context(0, *_ctx(911))
            s.set_context(1, *_ctx(912))
        outs_f, outs_m = run(3)
    finally:
        sess.close()
        ref_sess.close()
    total = 0
    for f, m in zip(outs_f, outs_m):
        if f is None:
            continue
        total += len(f)
        for c in range(2):
            assert _same(np.ascontiguousarray(f[:, c]), m[c])
    assert total > live.emitted(len(x), True, 48000, 48000) and len(short) > 10
