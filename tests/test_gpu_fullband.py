"""Full-band live output on the device (nhans_fullband_*, live.LiveSession.enable_fullband): the exact bypass, gain 0
against a session without the feature, the whole-clip twin against float64 and the float32 restatement, and every live
output BIT for bit that twin -- whatever the cutting, after rewind and restart, with a gain changed mid-stream, at
look-ahead 2, with the automatic wet factor, on interleaved frames --, the launch count of a push, the refusals and the
command line.  Seeded synthetic weights, two slots, recordings of 0.5 and 0.43 s with noise up to half the rate."""
import ctypes
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, resample, spec, synth

import fullband_checks as F

pytestmark = pytest.mark.gpu

PEAK = 21000
DENOM = PEAK + 0.000001
WET, G = 0.3, 0.7
# (rate, dtype in, dtype out)
CONFIGS = [(48000, np.int16, np.int16), (44100, np.float32, np.float32)]
CONFIG_IDS = ["48k_i16", "44k1_f32"]
RECS = [(931, 0.5), (932, 0.43)]          # slot -> (seed, seconds)
PRIMES = [7, 1009, 331, 13, 2003, 97, 4801, 2, 479, 163]


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    from nhans_amd import engine
    e = engine.Engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


_recs = {}


def _recording(rate, seed, seconds, dtype=np.int16):
    """synth.mixture(seed) brought to `rate` by interpolation, plus white noise: content up to rate / 2, int16 scale."""
    key = (rate, seed, seconds)
    if key not in _recs:
        base = synth.mixture(seed, seconds).astype(np.float64)
        n = int(len(base) * rate / 16000) - 37
        x = 0.6 * np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(base)), base)
        x = x + np.random.default_rng(seed).normal(0.0, 1500.0, n)
        _recs[key] = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(_recs[key].astype(dtype))


CTX_SEED = 931


def _ctx():
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(CTX_SEED))


_offline = {}


def _den_mix(e, rate, x, L=spec.LOOKAHEAD):
    """The offline 16 kHz results of a recording x at `rate`: computed once per recording, shared, never written to."""
    key = (rate, x.astype(np.float32).tobytes(), L)
    if key not in _offline:
        y = resample.resample(e, [x], rate, 16000)[0]
        m = apply.trim_to_frames(online.normalise_fixed(y, PEAK))
        ca, cb = _ctx()
        r = e.enhance([m], [ca], [cb], want_mixed=True, lookahead=L)
        den, mix = r["denoised_wav"][0], r["mixed_wav"][0]
        assert den.dtype == mix.dtype == np.float32 and len(den) == len(mix) == len(m)
        den.setflags(write=False); mix.setflags(write=False)
        _offline[key] = (den, mix)
    return _offline[key]


def _scale(dt_out):
    return live.default_out_scale(PEAK, dt_out)


def _want(e, rate, x, dt_out, wet=WET, g=G, L=spec.LOOKAHEAD, wet_hops=None):
    den, mix = _den_mix(e, rate, x, L)
    return live.fullband_mix(e, x, den, mix, rate, DENOM, wet=wet, gain=g, out_dtype=dt_out, out_scale=_scale(dt_out),
                             wet_hops=wet_hops)


def _cuts(kind, n, rate):
    if kind == "whole":
        return [n]
    if kind in ("10ms", "7ms"):
        k = rate * int(kind[:-2]) // 1000
        return [min(k, n - a) for a in range(0, n, k)]
    out, left, i = [], n, 0
    while left > 0:
        out.append(min(PRIMES[i % len(PRIMES)], left))
        left -= out[-1]
        i += 1
    return out


def _session(e, rate, dt_in, dt_out, n=2, L=spec.LOOKAHEAD, enable=True, wet=WET, g=G, **kw):
    s = live.LiveSession(e, n, rate, rate, PEAK, in_dtype=dt_in, out_dtype=dt_out, wet=True, lookahead=L, **kw)
    try:
        for i in range(s.S):
            s.set_context(i, *_ctx())
        s.set_wet(wet)
        if enable:
            s.enable_fullband()
            s.enable_fullband()
            if g is not None:
                s.set_highband(g)
    except Exception:
        s.close()
        raise
    return s


def _drive(sess, xs, cuts, before=None, rewind_at=()):
    """xs[i], cuts[i]: the recording stream i carries ([n] or [n, channels]) and its cutting; a stream that has ended
    gets empty pieces.  -> the concatenated output per stream."""
    n = sess.nstreams
    pos, k, outs, step = [0] * n, [0] * n, [[] for _ in range(n)], 0
    while any(k[i] < len(cuts[i]) for i in range(n)):
        chunks, end = [], []
        for i in range(n):
            live_ = k[i] < len(cuts[i])
            c = cuts[i][k[i]] if live_ else 0
            chunks.append(xs[i][pos[i]:pos[i] + c])
            end.append(live_ and k[i] == len(cuts[i]) - 1)
            pos[i] += c
            k[i] += 1 if live_ else 0
        if before is not None:
            before(step)
        got = sess.push(chunks, end)
        if step in rewind_at:
            sess.rewind()
            assert hip.load().nhans_live_rewind(sess.handle) == -1
            again = sess.push(chunks, end)
            for a, b in zip(got, again):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), step
        for i in range(n):
            outs[i].append(got[i])
        step += 1
    return [np.concatenate(o) for o in outs]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _two(rate, dtype):
    return [_recording(rate, seed, seconds, dtype) for seed, seconds in RECS]


# ---- the consequences of the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [48000, 44100])
def test_bypass_is_exact(eng, rate):
    """int16 in and out on the default scale, wet 1, gain 1: every emitted sample is the input sample of its index."""
    xs = _two(rate, np.int16)
    sess = _session(eng, rate, np.int16, np.int16, wet=1.0, g=None)
    try:
        outs = _drive(sess, xs, [_cuts("10ms", len(xs[0]), rate), _cuts("primes", len(xs[1]), rate)])
    finally:
        sess.close()
    for x, y in zip(xs, outs):
        assert y.dtype == np.int16 and len(y) == live.emitted(len(x), True, rate, rate) > len(x) * 9 // 10
        n = min(len(x), len(y))
        assert np.array_equal(y[:n], x[:n])
        assert not y[n:].any()                  # (outputs past the input, where the count rounds up: u = 0)
        assert np.abs(np.diff(x.astype(np.int32))).mean() > 500          # (a signal with a high band to lose)


SINKS = [("i16", np.int16, {}), ("f32", np.float32, {}), ("i16_split", np.int16, dict(channels=2, channel_mode="split")),
         ("f32_downmix", np.float32, dict(channels=2, out_channels=3))]


@pytest.mark.parametrize("name,dt_out,kw", SINKS, ids=[s[0] for s in SINKS])
def test_gain_zero_is_a_session_without_the_feature(eng, name, dt_out, kw):
    rate = 48000
    a, b = _recording(rate, 931, 0.5), _recording(rate, 933, 0.5)
    if kw:
        xs, n = [np.ascontiguousarray(np.stack([a, b], axis=1))], 1
    else:
        xs, n = [a, b], 2
    cuts = [_cuts("10ms", len(a), rate)] * n
    outs = []
    for enable in (False, True):
        sess = _session(eng, rate, np.int16, dt_out, n=n, enable=enable, g=0.0, **kw)
        try:
            outs.append(_drive(sess, xs, cuts))
        finally:
            sess.close()
    for p, q in zip(*outs):
        assert p.dtype == np.dtype(dt_out) and len(p) > 0.5 * len(a) and np.array_equal(p, q)


@pytest.mark.parametrize("rate", [48000, 44100])
def test_parity_with_float64(eng, rate):
    """The whole-clip twin, float32 out at scale 1, against the definition in float64 (resample_poly) and in float32 on
    the CPU, at the bar of one conversion chain: err_hip <= 1.5 * err_cpu32 + 1e-7 * peak.  Both restatements round e, u
    and the two sums as the device does; what differs is the chain's fused multiply-add."""
    x = _recording(rate, *RECS[0])
    den, mix = _den_mix(eng, rate, x)
    for wet, g in ((WET, G), (0.0, 1.0), (1.0, 4.0)):
        got = live.fullband_mix(eng, x, den, mix, rate, DENOM, wet=wet, gain=g, out_dtype=np.float32)
        y64 = F.restate64(x, den, mix, rate, DENOM, wet, g)
        y32 = F.add_high32(F.cpu32(F.residual32(den, mix, wet, g), rate), x, DENOM, g)
        assert got.dtype == np.float32 and len(got) == len(y64) == len(y32)
        err_hip, err_cpu, peak = float(np.abs(got - y64).max()), float(np.abs(y32 - y64).max()), float(np.abs(y64).max())
        print("fullband %d Hz wet %g g %g: err_hip %.3e  err_cpu32 %.3e  peak %.4e" % (rate, wet, g, err_hip, err_cpu, peak))
        assert err_hip <= 1.5 * err_cpu + 1e-7 * peak
    # the band is there: above 10 kHz the output has the input's spectrum, the plain conversion has none
    got = live.fullband_mix(eng, x, den, mix, rate, DENOM, wet=1.0, gain=1.0, out_dtype=np.float32)
    plain = live.fullband_mix(eng, x, den, mix, rate, DENOM, wet=1.0, gain=0.0, out_dtype=np.float32)
    n = min(len(got), len(x))
    hi = np.fft.rfftfreq(n, 1.0 / rate) > 10000.0
    spec_of = lambda v: np.abs(np.fft.rfft(v[:n].astype(np.float64)))[hi]
    assert F.rms(spec_of(plain)) < 1e-2 * F.rms(spec_of(x / DENOM))
    assert abs(F.rms(spec_of(got)) / F.rms(spec_of(x / DENOM)) - 1.0) < 1e-2


_runs = {}


def _scenario(e, config, kind):
    key = (CONFIGS.index(config), kind)
    if key not in _runs:
        rate, dt_in, dt_out = config
        xs = _two(rate, dt_in)
        sess = _session(e, rate, dt_in, dt_out)
        try:
            _runs[key] = _drive(sess, xs, [_cuts(kind, len(x), rate) for x in xs])
        finally:
            sess.close()
    return _runs[key]


@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_cutting_independence_bit_for_bit(eng, config):
    """Whole streams, 10 ms, 7 ms and prime-sized pieces: one output, that of the whole-clip twin -- which is the header's
    arithmetic operation for operation: numpy's float32 e, the device's plain conversion of it, numpy's lo + g u, the sink."""
    rate, dt_in, dt_out = config
    xs = _two(rate, dt_in)
    whole = _scenario(eng, config, "whole")
    for i, x in enumerate(xs):
        want = _want(eng, rate, x, dt_out)
        assert _same(whole[i], want), i
        for kind in ("10ms", "7ms", "primes"):
            assert _same(_scenario(eng, config, kind)[i], want), (kind, i)
        den, mix = _den_mix(eng, rate, x)
        lo = resample.resample(eng, [F.residual32(den, mix, WET, G)], 16000, rate)[0]
        assert np.array_equal(want, F.pcm(F.add_high32(lo, x, DENOM, G), dt_out, _scale(dt_out)))
        assert not np.array_equal(want, _want(eng, rate, x, dt_out, g=0.0))


def test_rewind_and_restart(eng):
    """Pushes undone and repeated give the same pieces and the same stream; a slot restarted mid-stream, and one restarted
    after its end, carry their next recording as a fresh slot would."""
    rate, dt_in, dt_out = CONFIGS[0]
    xs = _two(rate, dt_in)
    cuts = [_cuts("primes", len(x), rate) for x in xs]
    last = max(len(c) for c in cuts) - 1
    sess = _session(eng, rate, dt_in, dt_out)
    try:
        outs = _drive(sess, xs, cuts, rewind_at={0, 3, 4, 17, 30, 31, last - 1, last})
        for i, x in enumerate(xs):
            assert _same(outs[i], _want(eng, rate, x, dt_out)), i
        # slot 0 has ended; slot 1 gets a stream that is dropped half-way
        sess.restart(1)
        sess.push([np.zeros(0, dt_in), xs[0][:11000]])
        sess.push([np.zeros(0, dt_in), xs[0][11000:15000]])
        sess.restart(0)
        sess.restart(1)
        swapped = _drive(sess, xs[::-1], cuts[::-1], rewind_at={5, 12})
        for i, x in enumerate(xs[::-1]):
            assert _same(swapped[i], _want(eng, rate, x, dt_out)), i
    finally:
        sess.close()


def test_a_gain_changed_mid_stream_is_piecewise(eng):
    """set_highband(1.5, slot 0) before push 30 of 10 ms pieces: e[k] takes 1.5 from the first 16 kHz sample that push
    brings into the outgoing stage, g u[n] from the first output it emits; slot 1 keeps its gain."""
    rate, dt_in, dt_out = CONFIGS[0]
    xs = _two(rate, dt_in)
    cuts = [_cuts("10ms", len(x), rate) for x in xs]
    P, g1 = 30, 1.5
    sess = _session(eng, rate, dt_in, dt_out)
    try:
        outs = _drive(sess, xs, cuts, before=lambda step: sess.set_highband(g1, 0) if step == P else None)
    finally:
        sess.close()
    x = xs[0]
    den, mix = _den_mix(eng, rate, x)
    n_in = sum(cuts[0][:P])
    k = online.emitted(resample.emitted(n_in, False, rate, 16000), False)
    n = live.emitted(n_in, False, rate, rate)
    assert 0 < k < len(den) - 1000 and 0 < n < len(outs[0]) - 3000
    e = np.concatenate([F.residual32(den[:k], mix[:k], WET, G), F.residual32(den[k:], mix[k:], WET, g1)])
    lo = resample.resample(eng, [e], 16000, rate)[0]
    gv = np.where(np.arange(len(lo)) < n, np.float32(G), np.float32(g1)).astype(np.float32)
    y = lo + gv * F.u_of(x, DENOM, len(lo))
    assert y.dtype == np.float32
    assert _same(outs[0], F.pcm(y, dt_out, _scale(dt_out)))
    assert not _same(outs[0], _want(eng, rate, x, dt_out)) and not _same(outs[0], _want(eng, rate, x, dt_out, g=g1))
    assert _same(outs[1], _want(eng, rate, xs[1], dt_out))


@pytest.mark.parametrize("L,auto", [(2, False), (17, True), (2, True)], ids=["L2", "auto", "L2_auto"])
def test_lookahead_and_automatic_wet(eng, L, auto):
    """Look-ahead 2 (another hold occupancy, the same bound) and the per-hop factor of the level meter: bit for bit the
    twin on the offline results of that look-ahead, with level_gains' factors."""
    rate, dt_in, dt_out = CONFIGS[1]
    xs = _two(rate, dt_in)
    # (a clamp that decides some hops of slot 0's recording and not others: the median of its unclamped gains)
    wmax = float(np.median(live.level_gains(eng, *_den_mix(eng, rate, xs[0], L), 4, 1e9))) if auto else None
    sess = _session(eng, rate, dt_in, dt_out, L=L)
    try:
        if auto:
            sess.enable_levels()
            sess.set_auto_wet(4, wmax)
        outs = _drive(sess, xs, [_cuts("10ms", len(xs[0]), rate), _cuts("primes", len(xs[1]), rate)])
    finally:
        sess.close()
    for i, x in enumerate(xs):
        den, mix = _den_mix(eng, rate, x, L)
        hops = live.level_gains(eng, den, mix, 4, wmax) if auto else None
        if auto and i == 0:
            assert (hops == np.float32(wmax)).any() and (hops < np.float32(wmax)).any()
        assert _same(outs[i], _want(eng, rate, x, dt_out, L=L, wet_hops=hops)), i


@pytest.mark.parametrize("dt_out", [np.int16, np.float32], ids=["i16", "f32"])
def test_interleaved_sessions_equal_mono_sessions(eng, dt_out):
    """Split: the two channels of a stream are two mono slots.  Downmix: every output channel is the mono session fed
    live.downmix(frames), the high band being the downmix's."""
    rate = 48000
    a, b = _recording(rate, 931, 0.5), _recording(rate, 933, 0.5)
    frames = np.ascontiguousarray(np.stack([a, b], axis=1))
    cuts = _cuts("primes", len(a), rate)
    runs = {}
    for tag, dt_in, xs, kw in (("mono", np.int16, [a, b], dict(n=2)),
                               ("split", np.int16, [frames], dict(n=1, channels=2, channel_mode="split")),
                               ("mean", np.float32, [live.downmix(frames)], dict(n=1)),
                               ("downmix", np.int16, [frames], dict(n=1, channels=2, out_channels=3))):
        sess = _session(eng, rate, dt_in, dt_out, **kw)
        try:
            runs[tag] = _drive(sess, xs, [cuts] * len(xs), rewind_at={25})
        finally:
            sess.close()
    assert runs["split"][0].shape == (len(runs["mono"][0]), 2)
    for c in range(2):
        assert _same(np.ascontiguousarray(runs["split"][0][:, c]), runs["mono"][c]), c
    assert _same(runs["mono"][0], _want(eng, rate, a, dt_out))
    assert runs["downmix"][0].shape == (len(runs["mean"][0]), 3)
    for c in range(3):
        assert _same(np.ascontiguousarray(runs["downmix"][0][:, c]), runs["mean"][0]), c
    assert _same(runs["mean"][0], _want(eng, rate, live.downmix(frames), dt_out))


# ---- launches and refusals ------------------------------------------------------------------------------------------
def _steady_profiles(e, sess, x):
    profs = []
    for k, a in enumerate(range(0, len(x) - 960, 960)):
        steady = 12 <= k < 18
        if steady:
            e.set_option("profile", 1)
            e.profile_reset()
        try:
            got, = sess.push([x[a:a + 960]])
            if steady:
                profs.append({name: v["calls"] for name, v in e.profile().items()})
                assert len(got) == 960
        finally:
            if steady:
                e.set_option("profile", 0)
    assert len(profs) == 6
    return profs


def test_launches(eng):
    """20 ms pieces in the steady state: an object that never enabled the feature issues the launches of the parent
    commit, name for name and count for count (tests/golden/fullband_parent_launches.json: the same pushes on the parent
    commit's library), neither live_hold nor anything else new; an enabled one issues the same launches plus exactly one
    live_hold."""
    import json
    parent = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullband_parent_launches.json")))
    rate = 48000
    x = _recording(rate, *RECS[0])
    profs = {}
    for enable in (False, True):
        sess = _session(eng, rate, np.int16, np.int16, n=1, enable=enable)
        try:
            profs[enable] = _steady_profiles(eng, sess, x)
        finally:
            sess.close()
    for plain, full in zip(profs[False], profs[True]):
        assert plain == parent
        assert plain["live_in"] == 1 and plain["live_out"] == 1
        assert not any(k in plain for k in ("live_hold", "fullband_mix", "live_level"))
        assert full == dict(plain, live_hold=1)
        assert sum(full.values()) == sum(plain.values()) + 1


def test_refusals_change_nothing_and_launch_nothing(eng):
    lib = hip.load()
    rate, dt_in, dt_out = CONFIGS[0]
    x = _recording(rate, *RECS[0])
    cuts = _cuts("10ms", len(x), rate)
    eng.set_option("profile", 1)
    eng.profile_reset()

    def refused(rc, *words):
        assert rc == -1
        msg = lib.nhans_last_error()
        for w in words:
            assert w.encode() in msg, (w, msg)

    try:
        for rin, rout, wet, word in ((48000, 44100, True, "rates differ"), (16000, 16000, True, "16000 Hz"), (8000, 8000, True, "8000 Hz"),
                                     (48000, 48000, False, "NHANS_LIVE_WET")):
            s = live.LiveSession(eng, 1, rin, rout, PEAK, wet=wet)
            try:
                refused(lib.nhans_fullband_live_enable(s.handle, eng._stream()), "nhans_fullband_live_enable", word)
                refused(lib.nhans_fullband_live_set_gain(s.handle, 0, 1.0), "nhans_fullband_live_set_gain", "not enabled")
            finally:
                s.close()
        # a slot that has taken samples: refused, and the stream goes on as the plain stream it is
        sess = _session(eng, rate, dt_in, dt_out, n=1, enable=False)
        try:
            outs = [sess.push([x[:cuts[0]]])[0]]
            pushes = {k: v["calls"] for k, v in eng.profile().items()}
            refused(lib.nhans_fullband_live_enable(sess.handle, eng._stream()), "nhans_fullband_live_enable", "slot 0", "stream under way")
            with pytest.raises(hip.NhansError, match="nhans_fullband_live_enable"):
                sess.enable_fullband()
            assert {k: v["calls"] for k, v in eng.profile().items()} == pushes
            pos = cuts[0]
            for k, n in enumerate(cuts[1:]):
                outs.append(sess.push([x[pos:pos + n]], [k == len(cuts) - 2])[0])
                pos += n
            assert _same(np.concatenate(outs), _want(eng, rate, x, dt_out, g=0.0))
            # after a restart the slot has taken nothing: now it may
            sess.restart(0)
            sess.enable_fullband()
        finally:
            sess.close()
        # bad gains and slots on an enabled object: the gain stays what it was
        sess = _session(eng, rate, dt_in, dt_out, n=1)
        try:
            eng.profile_reset()
            for slot, g in ((0, float("nan")), (0, float("inf")), (0, -0.1), (0, 4.5), (1, 1.0), (-2, 1.0), (-1, 5.0)):
                refused(lib.nhans_fullband_live_set_gain(sess.handle, slot, g), "nhans_fullband_live_set_gain")
            with pytest.raises(hip.NhansError, match="nhans_fullband_live_set_gain"):
                sess.set_highband(7.0)
            assert not any(v["calls"] for v in eng.profile().values())
            eng.set_option("profile", 0)
            got, = _drive(sess, [x], [cuts])
            assert _same(got, _want(eng, rate, x, dt_out))
        finally:
            sess.close()
    finally:
        eng.set_option("profile", 0)
    den, mix = _den_mix(eng, rate, x)
    with pytest.raises(hip.NhansError, match="nhans_fullband_mix"):
        live.fullband_mix(eng, x, den, mix, 16000, DENOM)
    with pytest.raises(hip.NhansError, match="nhans_fullband_mix"):
        live.fullband_mix(eng, x, den, mix, rate, DENOM, gain=4.5)
    with pytest.raises(hip.NhansError, match="nhans_fullband_mix"):
        live.fullband_mix(eng, x, den, mix, rate, 0.0)


# ---- command line -----------------------------------------------------------------------------------------------------
def test_cli_highband(eng, tmp_path):
    """A 44.1 kHz stereo int16 file with --highband 1 --output_rate input --convert_on gpu: the denoised and the
    compensated file within the project's waveform bar (1e-3 RMS) of the float64 restatement on the 16 kHz files of a
    plain run, x the channel mean of the file and the divisor the front end's peak."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    rng = np.random.default_rng(77)
    base = 0.6 * resample_poly(synth.mixture(77, 1.2).astype(np.float64), 441, 160)
    left = base + rng.normal(0.0, 1200.0, len(base))
    stereo = np.clip(np.round(np.stack([left, 0.5 * left + rng.normal(0.0, 900.0, len(base))], axis=1)), -32768, 32767).astype(np.int16)
    d = str(tmp_path)
    wavfile.write(os.path.join(d, "a.wav"), 44100, stereo)
    wavfile.write(os.path.join(d, "neg.wav"), 16000, synth.noise_context(77))
    saved = dict(apply._engines)
    apply.set_engine(spec.DENOISER, eng)
    common = ["--input", os.path.join(d, "a.wav"), "--neg", os.path.join(d, "neg.wav"), "--pos", os.path.join(d, "Silent.wav"),
              "--weights", "synthetic", "--convert_on", "gpu", "--compensate", "0.25"]
    try:
        for tag, extra in (("plain", []), ("high", ["--output_rate", "input", "--highband", "1"])):
            os.makedirs(os.path.join(d, tag))
            apply.main(common + ["--output", os.path.join(d, tag, "a.wav")] + extra)
        with pytest.raises(SystemExit):
            apply.main(common + ["--output", os.path.join(d, "x.wav"), "--highband", "1"])
        in_denom = float(np.max(np.abs(apply.read_wav_any(os.path.join(d, "a.wav"))))) + 0.000001
    finally:
        apply._engines.clear()
        apply._engines.update(saved)
        apply.FLAGS.highband = None
        apply.FLAGS.convert_on = "host"
        apply.FLAGS.output_rate = "16000"
        apply.FLAGS.compensate = 0.0
    _, den = wavfile.read(os.path.join(d, "plain", "a.wav"))
    _, mix = wavfile.read(os.path.join(d, "plain", "a_mixed_processed.wav"))
    x = live.downmix(stereo)
    for fn, wet in (("a.wav", 0.0), ("a_compensated.wav", 0.25)):
        rate, got = wavfile.read(os.path.join(d, "high", fn))
        want = F.restate64(x, den, mix, 44100, in_denom, wet, 1.0)
        assert rate == 44100 and got.dtype == np.float32 and len(got) == len(want) == resample.out_count(len(den), 16000, 44100)
        err = F.rms(got - want)
        print("--highband 1 %s: RMS(file, float64 restatement) = %.3e, signal RMS %.3e" % (fn, err, F.rms(want)))
        assert err <= 1e-3
    # (the side files that carry no high band are the plain conversions they were)
    rate, got = wavfile.read(os.path.join(d, "high", "a_mixed_processed.wav"))
    assert rate == 44100 and np.array_equal(got, resample.resample(eng, [mix], 16000, 44100)[0])
