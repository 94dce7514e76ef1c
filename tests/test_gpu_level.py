"""Level meter and automatic compensation of live sessions on the device (nhans_level_*, n-hans_amd/live.py): the per-hop
gains against a float64 restatement, their independence of the cutting, the live output bit for bit the offline chain
with the per-hop factor, rewind, restart, switching between the fixed and the automatic factor, the launch count of a
push and the refusals.  Seeded synthetic weights, look-ahead 2, clips of 0.5 - 0.7 s, three slots of which slot 1 stays
idle and slot 2 ends half-way and carries a second recording."""
import ctypes
import struct

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, resample, synth

pytestmark = pytest.mark.gpu

PEAK = 21000
LA = 2
HOP = 160
# (rate in, dtype in, rate out, dtype out)
CONFIGS = [(48000, np.int16, 48000, np.int16), (44100, np.float32, 16000, np.float32)]
CONFIG_IDS = ["48k_i16-48k_i16", "44k1_f32-16k_f32"]
WINDOWS = [4, 0]
# slot -> the recordings it carries one after the other, (seed, seconds); slot 1 carries none
PLAN = {0: [(921, 0.7)], 1: [], 2: [(922, 0.5), (923, 0.6)]}
PRIMES = [7, 1009, 331, 13, 2003, 97, 4801, 2, 479, 163]


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    from nhans_amd import engine
    e = engine.Engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


def _recording(rate, seed, seconds, dtype):
    """`seconds` of synth.mixture(seed) on the int16 scale at `rate`, with a tail that fills no hop."""
    base = synth.mixture(seed, seconds)
    if rate == 48000:
        x = np.repeat(base, 3)[:-101]
    else:
        n = int(len(base) * rate / 16000) - 37
        x = np.round(np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(base)), base.astype(np.float64)))
    return np.ascontiguousarray(x.astype(dtype))


def _ctx(seed):
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(seed))


_offline = {}


def _den_mix(e, rate, dtype, seed, seconds):
    """The offline 16 kHz results of a recording at look-ahead LA: computed once, shared, never written to."""
    key = (rate, np.dtype(dtype).name, seed, seconds)
    if key not in _offline:
        y = resample.resample(e, [_recording(rate, seed, seconds, dtype)], rate, 16000)[0]
        m = apply.trim_to_frames(online.normalise_fixed(y, PEAK))
        ca, cb = _ctx(seed)
        r = e.enhance([m], [ca], [cb], want_mixed=True, lookahead=LA)
        den, mix = r["denoised_wav"][0], r["mixed_wav"][0]
        assert den.dtype == mix.dtype == np.float32 and len(den) == len(mix) == len(m) and len(den) % HOP == 80
        den.setflags(write=False); mix.setflags(write=False)
        _offline[key] = (den, mix)
    return _offline[key]


# ---- the definitions of include/nhans_hip.h in float64 (plain numpy sums: the order of a double sum is far below the bar)
def _powers64(den, mix):
    r = (mix - den).astype(np.float64)              # (float32 subtraction first: r is a float32 signal)
    assert (mix - den).dtype == np.float32
    nh = -(-len(den) // HOP)
    P = np.zeros((3, nh))
    for q, x in enumerate((den.astype(np.float64), r, mix.astype(np.float64))):
        for h in range(nh):
            P[q, h] = np.sum(x[HOP * h:HOP * h + HOP] ** 2)
    return P


def _sums64(P, W, h0=0):
    nh = P.shape[1]
    S = np.zeros((3, nh))
    for h in range(h0, nh):
        lo = h0 if W == 0 else max(h0, h - W + 1)
        S[:, h] = P[:, lo:h + 1].sum(axis=1)
    return S


def _gains64(den, mix, W, wmax):
    """-> (w_ref float64 per hop, decided: 'zero' where Sr == 0, 'clamp' where g is clearly beyond wmax, else None)."""
    S = _sums64(_powers64(den, mix), W)
    w, why = [], []
    for h in range(S.shape[1]):
        sd, sr = S[0, h], S[1, h]
        if sr == 0.0:
            w.append(0.0); why.append("zero")
            continue
        g = sd / sr / 20.0
        w.append(min(max(g, 0.0), wmax))
        why.append("clamp" if g > wmax * (1 + 1e-9) else None)
    return np.array(w), why


def _check_against_float64(w, den, mix, W, wmax):
    """The bar: |w - w_ref| <= 2^-23 max(w_ref, 1e-30) -- at most 160 * 256 exact products summed in double are within
    about 5e-12 relative of any other order, far below the one float32 rounding of w (2^-24) -- and equality where the
    clamp or the Sr == 0 rule decides.  (Measured on an MI355X: the largest |w - w_ref| / bar over all cases is 0.47.)"""
    ref, why = _gains64(den, mix, W, wmax)
    assert w.dtype == np.float32 and len(w) == len(ref)
    err = np.abs(w.astype(np.float64) - ref)
    bar = 2.0 ** -23 * np.maximum(ref, 1e-30)
    worst = int(np.argmax(err - bar))
    print("W=%d wmax=%g hops=%d: max |w - ref| / bar = %.3g (hop %d)" % (W, wmax, len(w), float(np.max(err / bar)), worst))
    assert (err <= bar).all(), (W, wmax, worst, float(w[worst]), float(ref[worst]))
    for h, y in enumerate(why):
        if y == "zero":
            assert w[h] == 0.0, h
        elif y == "clamp":
            assert w[h] == np.float32(wmax), h
    return ref, why


def _wmax_for(e, rate, dtype, seed, seconds, W):
    """A clamp that decides some hops and not others: the median of the float64 gain of the recording's hops."""
    den, mix = _den_mix(e, rate, dtype, seed, seconds)
    S = _sums64(_powers64(den, mix), W)
    g = S[0] / np.maximum(S[1], 1e-300) / 20.0
    return float(np.median(g))


def test_gains_against_float64(eng):
    """level_gains on offline den / mix, on a clip whose den == mix (gain 0 everywhere), on one whose removed part is
    tiny (the clamp everywhere), and on ragged seeded noise clips -- 1 sample, 80, 160, 161, more than two rounds of 256
    hops with a short tail -- for W = 0, 1, 4, 256."""
    rng = np.random.default_rng(77)
    den, mix = _den_mix(eng, 48000, np.int16, 921, 0.7)
    for W in (4, 0):
        wmax = _wmax_for(eng, 48000, np.int16, 921, 0.7, W)
        w = live.level_gains(eng, den, mix, W, wmax)
        ref, why = _check_against_float64(w, den, mix, W, wmax)
        assert why.count("clamp") >= 5 and sum(1 for h, y in enumerate(why) if y is None and 0 < ref[h] < wmax) >= 5
    w = live.level_gains(eng, den, den, 4, 1.0)
    assert len(w) == len(den) // HOP + 1
    _, why = _check_against_float64(w, den, den, 4, 1.0)
    assert why.count("zero") == len(w)
    near = (den * np.float32(1.0005)).astype(np.float32)
    w = live.level_gains(eng, den, near, 4, 0.75)
    _, why = _check_against_float64(w, den, near, 4, 0.75)
    assert why.count("clamp") >= len(w) - 4 and (w == np.float32(0.75)).sum() >= len(w) - 4
    lens = [1, 80, 160, 161, HOP * 600 + 37, 0, HOP * 256, HOP * 257 - 1]
    dens = [rng.standard_normal(n).astype(np.float32) for n in lens]
    mixes = [(d + rng.standard_normal(len(d)).astype(np.float32) * np.float32(0.2)).astype(np.float32) for d in dens]
    mixes[2] = dens[2].copy()
    for W in (0, 1, 4, 256):
        got, sums = live.level_gains(eng, dens, mixes, W, 2.0, sums=True)
        for i, n in enumerate(lens):
            assert len(got[i]) == live.level_hops(n, True)
            if n == 0:
                continue
            _check_against_float64(got[i], dens[i], mixes[i], W, 2.0)
            S = _sums64(_powers64(dens[i], mixes[i]), W)[:, -1]
            assert np.allclose(sums[i][:3], S, rtol=1e-11, atol=0) and sums[i][3] == len(got[i])
            assert sums[i][4] == got[i][-1] and sums[i][6] == sums[i][7] == 0
            assert sums[i][5] == sums[i][0] / sums[i][1] if sums[i][1] else not np.isfinite(sums[i][5])


# ---- live sessions ------------------------------------------------------------------------------------------------
def _pcm(y, out_dtype, scale):
    v = (y.astype(np.float64) * scale).astype(np.float32)
    if np.dtype(out_dtype) == np.float32:
        return v
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def _chain(e, den, mix, w_hops, out_rate, out_dtype, scale):
    """The offline chain with a per-hop factor: c on the host in float32, three separately rounded numpy operations,
    resample.resample of c, then the PCM sink's arithmetic."""
    w = np.repeat(np.asarray(w_hops, dtype=np.float32), HOP)[:len(den)]
    assert len(w) == len(den)
    c = den + (mix - den) * w
    assert c.dtype == np.float32
    return _pcm(resample.resample(e, [c], 16000, out_rate)[0], out_dtype, scale)


def _scale(out_dtype):
    return live.default_out_scale(PEAK, out_dtype)


def _cuts(kind, n, rate):
    if kind == "whole":
        return [n]
    if kind == "10ms":
        k = rate // 100
        return [min(k, n - a) for a in range(0, n, k)]
    out, left, i = [], n, 0
    while left > 0:
        out.append(min(PRIMES[i % len(PRIMES)], left))
        left -= out[-1]
        i += 1
    return out


def _bits(levels):
    return struct.pack("<9d", *[float(levels[k]) for k in ("sd", "sr", "sm", "hops", "w", "snr_est", "denoised_dbfs",
                                                            "removed_dbfs", "mixed_dbfs")])


def _drive(sess, plan, before_push=None):
    """plan[i]: the recordings slot i carries one after the other, dict(x, cuts, ctx).  A slot whose recording has ended
    is restarted and conditioned for its next one.  -> per slot and recording dict(pcm, gains, levels: {hops: bits of
    levels() after the push that made that hop the last final one})."""
    S = sess.S
    queue = [list(p) for p in plan]
    now = [None] * S
    done = [[] for _ in range(S)]
    step = 0
    while any(queue) or any(n is not None for n in now):
        for i in range(S):
            if now[i] is None and queue[i]:
                now[i] = dict(queue[i].pop(0), pos=0, k=0, pcm=[], gains=[], levels={})
                sess.restart(i)
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
            before_push(step)
        got = sess.push(chunks, end)
        for i in range(S):
            r = now[i]
            if r is None:
                assert len(got[i]) == 0 and len(sess.last_gains(i)) == 0
                continue
            r["pcm"].append(got[i])
            g = sess.last_gains(i)
            r["gains"].append(g)
            if len(g):
                lv = sess.levels(i)
                assert lv["hops"] == sum(len(v) for v in r["gains"]) and np.float32(lv["w"]) == g[-1]
                r["levels"][lv["hops"]] = _bits(lv)
            if end[i]:
                assert r["pos"] == len(r["x"])
                done[i].append(dict(pcm=np.concatenate(r["pcm"]), gains=np.concatenate(r["gains"]), levels=r["levels"]))
                now[i] = None
        step += 1
    return done


_runs = {}


def _scenario(e, config, W, kind):
    """The three-slot scenario of PLAN on one cutting, automatic from the first hop: run once, shared."""
    key = (CONFIGS.index(config), W, kind)
    if key not in _runs:
        rate_in, dt_in, rate_out, dt_out = config
        plan = []
        for i in range(3):
            plan.append([])
            for seed, seconds in PLAN[i]:
                x = _recording(rate_in, seed, seconds, dt_in)
                plan[i].append(dict(x=x, cuts=_cuts(kind, len(x), rate_in), ctx=_ctx(seed)))
        wmax = _wmax_for(e, rate_in, dt_in, *PLAN[0][0], W)
        sess = live.LiveSession(e, 3, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, wet=True, lookahead=LA)
        try:
            with pytest.raises(hip.NhansError, match="nhans_level_live_auto"):
                sess.set_auto_wet(W, wmax)                  # (not before the meter is enabled)
            sess.enable_levels()
            sess.enable_levels()
            sess.set_auto_wet(W, wmax)
            done = _drive(sess, plan)
            with pytest.raises(hip.NhansError) as err:      # slot 1 never had a hop
                sess.levels(1)
            assert err.value.code == hip.ESHORT
        finally:
            sess.close()
        _runs[key] = (done, wmax)
    return _runs[key]


def _expected(e, config, W, wmax, seed, seconds):
    rate_in, dt_in, rate_out, dt_out = config
    den, mix = _den_mix(e, rate_in, dt_in, seed, seconds)
    w, sums = live.level_gains(e, den, mix, W, wmax, sums=True)
    return w, sums, _chain(e, den, mix, w, rate_out, dt_out, _scale(dt_out))


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_cutting_independence_bit_for_bit(eng, config, W):
    """The same streams pushed whole, in 10 ms pieces and in pieces of irregular prime lengths: identical PCM, identical
    per-hop gains, identical levels() wherever two cuttings stop at the same hop -- at every stream's end at least."""
    whole, wmax = _scenario(eng, config, W, "whole")
    for kind in ("10ms", "primes"):
        other, _ = _scenario(eng, config, W, kind)
        for i in range(3):
            assert len(other[i]) == len(whole[i]) == len(PLAN[i])
            for a, b in zip(whole[i], other[i]):
                assert a["pcm"].dtype == b["pcm"].dtype and a["pcm"].tobytes() == b["pcm"].tobytes(), (kind, i)
                assert a["gains"].tobytes() == b["gains"].tobytes(), (kind, i)
                last = len(a["gains"])
                assert last in a["levels"] and last in b["levels"]
                for h in set(a["levels"]) & set(b["levels"]):
                    assert a["levels"][h] == b["levels"][h], (kind, i, h)
    ten, _ = _scenario(eng, config, W, "10ms")
    primes, _ = _scenario(eng, config, W, "primes")
    shared = set(ten[0][0]["levels"]) & set(primes[0][0]["levels"])
    assert len(shared) >= 3                                 # (mid-stream hops too, not only the end)
    for h in shared:
        assert ten[0][0]["levels"][h] == primes[0][0]["levels"][h]
    gains = whole[0][0]["gains"]
    assert len(gains) > 4 * max(W, 1) + 20 and (gains == np.float32(wmax)).any() and ((gains > 0) & (gains < np.float32(wmax))).any()


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_bit_for_bit_the_offline_chain(eng, config, W):
    """The 10 ms cutting against the offline statement: gains == level_gains of the offline den / mix, the meter at each
    stream's end == its sums, and the PCM == resample(den + (mix - den) * w per hop) through the sink's arithmetic.  The
    restarted slot's second recording included: h0 is 0 again and nothing of the first stream's state is read."""
    done, wmax = _scenario(eng, config, W, "10ms")
    for i in range(3):
        for k, (seed, seconds) in enumerate(PLAN[i]):
            w, sums, want = _expected(eng, config, W, wmax, seed, seconds)
            got = done[i][k]
            assert got["gains"].tobytes() == w.tobytes(), (i, k)
            assert got["pcm"].dtype == want.dtype and np.array_equal(got["pcm"], want), (i, k)
            end = struct.unpack("<9d", got["levels"][len(w)])
            assert struct.pack("<6d", *end[:6]) == struct.pack("<6d", *sums[:6]), (i, k)
    # (the factor matters: the fixed-factor outputs differ)
    seed, seconds = PLAN[0][0]
    den, mix = _den_mix(eng, config[0], config[1], seed, seconds)
    flat = _chain(eng, den, mix, np.zeros(len(den) // HOP + 1, np.float32), config[2], config[3], _scale(config[3]))
    assert not np.array_equal(done[0][0]["pcm"], flat)


def test_a_restarted_slot_equals_a_fresh_object(eng):
    """Slot 2's second recording in the three-slot scenario against the same recording alone in a fresh one-slot object."""
    config, W = CONFIGS[0], 4
    done, wmax = _scenario(eng, config, W, "primes")
    seed, seconds = PLAN[2][1]
    x = _recording(config[0], seed, seconds, config[1])
    sess = live.LiveSession(eng, 1, config[0], config[2], PEAK, in_dtype=config[1], out_dtype=config[3], wet=True, lookahead=LA)
    try:
        sess.enable_levels()
        sess.set_auto_wet(W, wmax)
        fresh, = _drive(sess, [[dict(x=x, cuts=_cuts("10ms", len(x), config[0]), ctx=_ctx(seed))]])
    finally:
        sess.close()
    assert fresh[0]["gains"].tobytes() == done[2][1]["gains"].tobytes()
    assert fresh[0]["pcm"].tobytes() == done[2][1]["pcm"].tobytes()
    assert fresh[0]["levels"][len(fresh[0]["gains"])] == done[2][1]["levels"][len(fresh[0]["gains"])]


def _single(e, config, W, wmax, seed, seconds):
    rate_in, dt_in, rate_out, dt_out = config
    sess = live.LiveSession(e, 1, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, wet=True, lookahead=LA)
    sess.set_context(0, *_ctx(seed))
    sess.enable_levels()
    if W is not None:
        sess.set_auto_wet(W, wmax)
    return sess, _recording(rate_in, seed, seconds, dt_in)


def test_rewind(eng):
    """Push, rewind, push the same piece: every output, gain and meter reading as if never rewound.  Push, rewind, push
    a different piece: the run of that cutting."""
    config, W = CONFIGS[0], 4
    seed, seconds = PLAN[0][0]
    wmax = _wmax_for(eng, config[0], config[1], seed, seconds, W)
    w, sums, want = _expected(eng, config, W, wmax, seed, seconds)
    lib = hip.load()
    sess, x = _single(eng, config, W, wmax, seed, seconds)
    try:
        cuts = _cuts("primes", len(x), config[0])
        outs, gains, pos = [], [], 0
        emitting = 0
        for k, n in enumerate(cuts):
            piece, end = x[pos:pos + n], [k == len(cuts) - 1]
            got, = sess.push([piece], end)
            g = sess.last_gains(0)
            lv = _bits(sess.levels(0)) if len(g) else None
            if len(g) and emitting % 2 == 0 or end[0] or k == 0:
                sess.rewind()
                assert lib.nhans_live_rewind(sess.handle) == -1
                assert len(sess.last_gains(0)) == 0
                again, = sess.push([piece], end)
                assert again.tobytes() == got.tobytes() and sess.last_gains(0).tobytes() == g.tobytes(), k
                assert lv is None or _bits(sess.levels(0)) == lv, k
            emitting += 1 if len(g) else 0
            outs.append(got); gains.append(g)
            pos += n
        assert emitting >= 6
        assert np.concatenate(gains).tobytes() == w.tobytes()
        assert np.array_equal(np.concatenate(outs), want)
    finally:
        sess.close()
    # a different piece after the rewind
    sess, x = _single(eng, config, W, wmax, seed, seconds)
    try:
        outs, gains = [], []
        first = 9600
        a, = sess.push([x[:first]])
        assert len(sess.last_gains(0)) > 0
        outs.append(a); gains.append(sess.last_gains(0))
        sess.push([x[first:first + 4800]])
        assert len(sess.last_gains(0)) > 0
        sess.rewind()
        pos = first
        for n in [1009, 4801] + _cuts("10ms", len(x) - first - 1009 - 4801, config[0]):
            got, = sess.push([x[pos:pos + n]], [pos + n == len(x)])
            outs.append(got); gains.append(sess.last_gains(0))
            pos += n
        assert pos == len(x)
        assert np.concatenate(gains).tobytes() == w.tobytes()
        assert np.array_equal(np.concatenate(outs), want)
        assert struct.pack("<6d", *struct.unpack("<9d", _bits(sess.levels(0)))[:6]) == struct.pack("<6d", *sums[:6])
    finally:
        sess.close()


def test_switching_between_fixed_and_automatic(eng):
    """Automatic from the start; set_wet(0.5) at push 10 changes nothing while automatic; set_auto_wet(None) at push 20
    returns to the stored 0.5 from the next final hop on; set_auto_wet(W, wmax) at push 35 resumes the law, whose window
    has gone on metering meanwhile.  The output is the conversion of that piecewise c."""
    config, W = CONFIGS[0], 4
    rate_in, dt_in, rate_out, dt_out = config
    seed, seconds = PLAN[0][0]
    wmax = _wmax_for(eng, rate_in, dt_in, seed, seconds, W)
    den, mix = _den_mix(eng, rate_in, dt_in, seed, seconds)
    w = live.level_gains(eng, den, mix, W, wmax)
    sess, x = _single(eng, config, W, wmax, seed, seconds)
    cuts = _cuts("10ms", len(x), rate_in)
    assert len(cuts) > 50

    def hops_before(step):
        n16 = resample.emitted(sum(cuts[:step]), False, rate_in, 16000)
        return live.level_hops(online.emitted(n16, False, LA), False)

    h_off, h_on = hops_before(20), hops_before(35)
    assert 0 < hops_before(10) < h_off < h_on < len(w) - 5
    piecewise = w.copy()
    piecewise[h_off:h_on] = np.float32(0.5)
    assert not np.array_equal(piecewise, w)
    want = _chain(eng, den, mix, piecewise, rate_out, dt_out, _scale(dt_out))

    def before(step):
        if step == 10:
            sess.set_wet(0.5)
        elif step == 20:
            sess.set_auto_wet(None)
        elif step == 35:
            sess.set_auto_wet(W, wmax)

    try:
        outs, gains, pos = [], [], 0
        for k, n in enumerate(cuts):
            before(k)
            got, = sess.push([x[pos:pos + n]], [k == len(cuts) - 1])
            outs.append(got); gains.append(sess.last_gains(0))
            pos += n
    finally:
        sess.close()
    assert np.concatenate(gains).tobytes() == w.tobytes()          # (the law's gains, applied or not)
    assert np.array_equal(np.concatenate(outs), want)


@pytest.mark.parametrize("W", WINDOWS)
def test_enabled_mid_stream(eng, W):
    """enable_levels() before push 15 of a running stream: h0 is the hop count then, the sums start there -- against the
    float64 restatement with that h0, at the bar of test_gains_against_float64 -- and the hops before it keep the fixed
    factor's output."""
    config = CONFIGS[0]
    rate_in, dt_in, rate_out, dt_out = config
    seed, seconds = PLAN[0][0]
    den, mix = _den_mix(eng, rate_in, dt_in, seed, seconds)
    x = _recording(rate_in, seed, seconds, dt_in)
    cuts = _cuts("10ms", len(x), rate_in)
    h0 = live.level_hops(online.emitted(resample.emitted(sum(cuts[:15]), False, rate_in, 16000), False, LA), False)
    assert 4 < h0 < len(den) // HOP - 20
    S = _sums64(_powers64(den, mix), W, h0)[:, h0:]
    ref = np.where(S[1] == 0, 0.0, np.clip(S[0] / np.maximum(S[1], 1e-300) / 20.0, 0.0, 1e9))
    sess = live.LiveSession(eng, 1, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, wet=True, lookahead=LA)
    try:
        sess.set_context(0, *_ctx(seed))
        outs, gains, pos = [], [], 0
        for k, n in enumerate(cuts):
            if k == 15:
                sess.enable_levels()
                sess.set_auto_wet(W, 1e9)
            outs.append(sess.push([x[pos:pos + n]], [k == len(cuts) - 1])[0])
            if k >= 15:
                gains.append(sess.last_gains(0))
            pos += n
        lv = sess.levels(0)
    finally:
        sess.close()
    w = np.concatenate(gains)
    assert len(w) == len(ref) == lv["hops"] and np.float32(lv["w"]) == w[-1]
    err = np.abs(w.astype(np.float64) - ref)
    assert (err <= 2.0 ** -23 * np.maximum(ref, 1e-30)).all(), float(np.max(err / np.maximum(ref, 1e-30)))
    full = np.concatenate([np.zeros(h0, np.float32), w])
    assert np.array_equal(np.concatenate(outs), _chain(eng, den, mix, full, rate_out, dt_out, _scale(dt_out)))


def test_a_fixed_factor_that_is_no_power_of_two(eng):
    """set_wet(0.3) on an object that never enables its meter: c = den + (mix - den) * float32(0.3) in three separately
    rounded operations, as the header says -- a product fused into the sum rounds once and differs in the last bit of
    some samples, which the factors 0.25 and 0.5 (exact products) cannot show."""
    for config in CONFIGS:
        rate_in, dt_in, rate_out, dt_out = config
        seed, seconds = PLAN[0][0]
        den, mix = _den_mix(eng, rate_in, dt_in, seed, seconds)
        want = _chain(eng, den, mix, np.full(len(den) // HOP + 1, 0.3, np.float32), rate_out, dt_out, _scale(dt_out))
        x = _recording(rate_in, seed, seconds, dt_in)
        sess = live.LiveSession(eng, 1, rate_in, rate_out, PEAK, in_dtype=dt_in, out_dtype=dt_out, wet=True, lookahead=LA)
        try:
            sess.set_context(0, *_ctx(seed))
            sess.set_wet(0.3)
            outs, pos = [], 0
            cuts = _cuts("primes", len(x), rate_in)
            for k, n in enumerate(cuts):
                outs.append(sess.push([x[pos:pos + n]], [k == len(cuts) - 1])[0])
                pos += n
        finally:
            sess.close()
        assert np.array_equal(np.concatenate(outs), want), config


def test_launches(eng):
    """20 ms pieces in the steady state, where every push makes two hops final: live_level is in the profile 0 times per
    push on an object that never enabled its meter and exactly once per push after enable_levels(), automatic or not;
    live_out once per push in every case."""
    config = CONFIGS[0]
    seed, seconds = PLAN[0][0]
    for mode in ("never", "enabled", "auto"):
        sess = live.LiveSession(eng, 1, config[0], config[2], PEAK, wet=True, lookahead=LA)
        x = _recording(config[0], seed, seconds, config[1])
        profs = []
        try:
            sess.set_context(0, *_ctx(seed))
            sess.set_wet(0.25)
            if mode != "never":
                sess.enable_levels()
            if mode == "auto":
                sess.set_auto_wet(4, 1.0)
            for k, a in enumerate(range(0, len(x) - 960, 960)):
                steady = 12 <= k < 20
                if steady:
                    eng.set_option("profile", 1)
                    eng.profile_reset()
                try:
                    got, = sess.push([x[a:a + 960]])
                    if steady:
                        profs.append(eng.profile())
                        assert len(got) == 960
                finally:
                    if steady:
                        eng.set_option("profile", 0)
        finally:
            sess.close()
        assert len(profs) == 8
        for p in profs:
            assert p["live_in"]["calls"] == 1 and p["live_out"]["calls"] == 1, mode
            assert p.get("live_level", {"calls": 0})["calls"] == (0 if mode == "never" else 1), mode


def test_refusals_leave_the_object_usable(eng):
    """Enable without NHANS_LIVE_WET, W = 257, W = -2, wmax NaN / negative, read before the first hop: the documented
    code, the function's name in the message, and the stream's output still bit for bit the chain."""
    lib = hip.load()
    config, W = CONFIGS[0], 4
    rate_in, dt_in, rate_out, dt_out = config
    seed, seconds = PLAN[0][0]
    wmax = _wmax_for(eng, rate_in, dt_in, seed, seconds, W)
    _, _, want = _expected(eng, config, W, wmax, seed, seconds)
    dry = live.LiveSession(eng, 1, rate_in, rate_out, PEAK, lookahead=LA)
    try:
        assert lib.nhans_level_live_enable(dry.handle, eng._stream()) == -1
        assert b"nhans_level_live_enable" in lib.nhans_last_error() and b"NHANS_LIVE_WET" in lib.nhans_last_error()
        out = (ctypes.c_double * 8)()
        assert lib.nhans_level_live_read(dry.handle, 0, out, eng._stream()) == -1
        assert b"nhans_level_live_read" in lib.nhans_last_error()
    finally:
        dry.close()
    sess, x = _single(eng, config, W, wmax, seed, seconds)
    out = (ctypes.c_double * 8)()

    def bad():
        for args in ((257, 1.0), (-2, 1.0), (4, float("nan")), (4, float("inf")), (4, -0.5), (-1, float("nan"))):
            assert lib.nhans_level_live_auto(sess.handle, *args) == -1, args
            assert b"nhans_level_live_auto" in lib.nhans_last_error()
        assert lib.nhans_level_live_read(sess.handle, 1, out, eng._stream()) == -1
        assert b"nhans_level_live_read" in lib.nhans_last_error()
        assert lib.nhans_level_live_read(sess.handle, 0, None, eng._stream()) == -1
        assert lib.nhans_level_live_gains(sess.handle, 1, None, 0, eng._stream()) == -1
        assert b"nhans_level_live_gains: slot 1 outside" in lib.nhans_last_error()

    def short_room():
        """Room for one gain fewer than the last push made final: the status, not a count."""
        n = lib.nhans_level_live_gains(sess.handle, 0, None, 0, eng._stream())
        if n > 0:
            room = (ctypes.c_float * n)()
            assert lib.nhans_level_live_gains(sess.handle, 0, room, n - 1, eng._stream()) == -1
            assert lib.nhans_last_error() == b"nhans_level_live_gains: room for %d gains, %d needed" % (n - 1, n)
            assert lib.nhans_level_live_gains(sess.handle, 0, room, n, eng._stream()) == n
        return n > 0

    try:
        bad()
        assert lib.nhans_level_live_read(sess.handle, 0, out, eng._stream()) == hip.ESHORT
        assert b"nhans_level_live_read" in lib.nhans_last_error()
        with pytest.raises(hip.NhansError) as err:
            sess.levels(0)
        assert err.value.code == hip.ESHORT
        outs, pos, short = [], 0, 0
        cuts = _cuts("primes", len(x), rate_in)
        for k, n in enumerate(cuts):
            if k % 3 == 0:
                bad()
            got, = sess.push([x[pos:pos + n]], [k == len(cuts) - 1])
            outs.append(got)
            pos += n
            short += short_room()
        assert short > 0
        assert sess.levels(0)["hops"] == len(want) * 16000 // rate_out // HOP + 1
    finally:
        sess.close()
    assert np.array_equal(np.concatenate(outs), want)
    assert lib.nhans_level_gains(eng.handle, None, None, hip.i64_array([0, 160]), 1, 257, 1.0, None, None, eng._stream()) == -1
    assert b"nhans_level_gains" in lib.nhans_last_error()
    assert lib.nhans_level_gains(eng.handle, None, None, hip.i64_array([0, 160]), 1, 4, 1.0, None, None, eng._stream()) == -1
    assert b"nhans_level_gains" in lib.nhans_last_error()
