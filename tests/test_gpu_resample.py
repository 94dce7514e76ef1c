"""Sample-rate conversion on the device (nhans_resample, nhans_resampler_*, nhans_peak_normalise; n-hans_amd/resample.py):
accuracy against scipy.signal.resample_poly in float64, the quantised output, streams cut into pieces against the
conversion of the whole (bit for bit), the peak normalisation against apply.normalise (bit for bit), and a live 48 kHz
int16 recording through OnlineEnhancer(in_rate, out_rate) against the offline chain (bit for bit, both engines)."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, online, resample, spec, synth
# (no torch at import time: the torch-free worker below is unpickled from this module in a fresh process)

pytestmark = pytest.mark.gpu

OTHER = [r for r in resample.RATES if r != 16000]
PAIRS = [(r, 16000) for r in OTHER] + [(16000, r) for r in OTHER]
IDS = ["%d-%d" % p for p in PAIRS]


def _engine(*args, **kw):
    from nhans_amd import engine
    return engine.Engine(*args, **kw)


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


def _ref64(x, pair):
    from scipy.signal import resample_poly
    L, M, _, _ = resample.geometry(*pair)
    if len(x) == 0:
        return np.zeros(0)
    return resample_poly(np.asarray(x, np.float64), L, M)


def _cpu32(x, pair):
    """The float32 restatement of y[m] on the CPU: taps rounded to float32, one sequential float32 accumulation per
    output (multiply, round, add, round), taps in the kernel's order."""
    L, M, half, J = resample.geometry(*pair)
    h = np.zeros(L * J, np.float32)
    t = resample.taps(*pair).astype(np.float32)
    h[:len(t)] = t
    n = len(x)
    m = np.arange(resample.out_count(n, *pair), dtype=np.int64)
    q, p = np.divmod(m * M + half, L)
    xp = np.concatenate([np.zeros(J, np.float32), np.asarray(x, np.float32), np.zeros(J + half // L + 2, np.float32)])
    acc = np.zeros(len(m), np.float32)
    for j in range(J):
        k = q - j
        xv = np.where((k >= 0) & (k < n), xp[np.clip(k, -J, n + J) + J], np.float32(0))
        acc = (h[p + j * L] * xv).astype(np.float32) + acc
    return acc


def _signals(pair, seed):
    """int16-scale test clips at pair[0] Hz: noise, a swept sine, a clip that starts and ends at full scale, and the
    ragged edge cases (0, 1 and J - 1 samples)."""
    rate = pair[0]
    J = resample.geometry(*pair)[3]
    rng = np.random.default_rng(seed)
    n = int(0.2 * rate) + 13
    noise = rng.integers(-32768, 32768, n).astype(np.int16)
    tt = np.arange(n) / rate
    sweep = np.round(30000 * np.sin(2 * np.pi * (50 * tt + 0.5 * (0.45 * rate / tt[-1]) * tt * tt))).astype(np.int16)
    full = np.round(20000 * np.sin(2 * np.pi * 300 * tt)).astype(np.int16)
    full[:40] = 32767
    full[-40:] = -32768
    return [noise, np.zeros(0, np.int16), sweep, noise[:1].copy(), full, noise[5:5 + J - 1].copy()]


_measured = {}


def _measure(eng, pair):
    """-> (clips, float64 references, device outputs, err_hip, err_cpu32, peak), once per pair"""
    if pair not in _measured:
        clips = _signals(pair, 1000 + PAIRS.index(pair))
        refs = [_ref64(c, pair) for c in clips]
        got = resample.resample(eng, clips, pair[0], pair[1])
        for g, r, c in zip(got, refs, clips):
            assert g.dtype == np.float32 and len(g) == len(r) == resample.out_count(len(c), *pair)
        err_hip = max(float(np.abs(g - r).max()) for g, r in zip(got, refs) if len(r))
        err_cpu = max(float(np.abs(_cpu32(c, pair) - r).max()) for c, r in zip(clips, refs) if len(r))
        peak = max(float(np.abs(r).max()) for r in refs if len(r))
        _measured[pair] = (clips, refs, got, err_hip, err_cpu, peak)
    return _measured[pair]


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_accuracy_against_resample_poly(eng, pair):
    """err_hip <= 1.5 * err_cpu32 + 1e-7 * peak: the device chain and the CPU float32 restatement are two float32
    rounding chains over the same taps (fused against unfused multiply-add), both measured against float64."""
    clips, refs, got, err_hip, err_cpu, peak = _measure(eng, pair)
    print("resample %d -> %d: err_hip %.3e  err_cpu32 %.3e  peak %.4e" % (pair[0], pair[1], err_hip, err_cpu, peak))
    assert err_hip <= 1.5 * err_cpu + 1e-7 * peak
    # float32 input of the same values: the same bits
    gotf = resample.resample(eng, [c.astype(np.float32) for c in clips], pair[0], pair[1])
    for a, b in zip(got, gotf):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_quantised_output(eng, pair):
    """With quantise every sample is within 1 LSB of np.round(resample_poly), and every sample that differs is a
    near-tie: its float64 value lies within the measured err_hip of n + 0.5.  No share of samples is exempt."""
    clips, refs, _, err_hip, _, _ = _measure(eng, pair)
    got = resample.resample(eng, clips, pair[0], pair[1], quantise=True)
    differ = total = 0
    for g, r in zip(got, refs):
        want = np.clip(np.round(r), -32768, 32767)
        assert np.array_equal(g, np.round(g)) and (len(g) == 0 or (g.min() >= -32768 and g.max() <= 32767))
        d = g.astype(np.float64) - want
        assert len(d) == 0 or np.abs(d).max() <= 1
        bad = d != 0
        frac = r[bad] - np.floor(r[bad])
        assert np.all(np.abs(frac - 0.5) <= err_hip), (pair, float(np.abs(frac - 0.5).max()), err_hip)
        differ += int(bad.sum())
        total += len(d)
    print("quantised %d -> %d: %d of %d samples differ from the float64 rounding (all near-ties)" % (pair[0], pair[1], differ, total))


def _cut(rng, n):
    out, left = [], n
    while left > 0:
        k = min(int(rng.choice([0, 1, 7, 160, 441, 480, 4800])), left)
        out.append(k)
        left -= k
    return out


def _drive(rs, xs, cuts, pair, restart_slot=None, second=None, second_cut=None):
    """Pushes stream i's pieces cuts[i] (ended streams push nothing); when restart_slot has ended it is restarted and
    `second` is pushed through it.  Checks every push's counts; returns the concatenated outputs (+ the second's)."""
    S = len(xs)
    xs, cuts = list(xs), [list(c) for c in cuts]
    pos, step, ended = [0] * S, [0] * S, [False] * S
    outs = [[] for _ in range(S)]
    first_of_slot = None
    reused = restart_slot is None
    while not all(ended):
        chunks, end = [], []
        for i in range(S):
            if ended[i]:
                chunks.append(xs[i][:0]); end.append(False)
                continue
            k = cuts[i][step[i]]
            step[i] += 1
            chunks.append(xs[i][pos[i]:pos[i] + k])
            end.append(step[i] == len(cuts[i]))
        before, was = list(rs.pushed), list(rs.ended)
        want = [resample.emitted(before[i] + len(chunks[i]), bool(end[i] or was[i]), *pair) - resample.emitted(before[i], was[i], *pair)
                for i in range(S)]
        assert rs.out_counts([len(c) for c in chunks], end) == want
        got = rs.push(chunks, end)
        for i in range(S):
            assert len(got[i]) == want[i]
            outs[i].append(got[i])
            pos[i] += len(chunks[i])
            ended[i] = ended[i] or end[i]
        if not reused and ended[restart_slot]:
            reused = True
            i = restart_slot
            first_of_slot = np.concatenate(outs[i])
            rs.restart(i)
            xs[i], cuts[i], pos[i], step[i], ended[i], outs[i] = second, list(second_cut), 0, 0, False, []
    return [np.concatenate(o) if o else np.zeros(0, np.float32) for o in outs], first_of_slot


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_streams_equal_the_whole_bit_for_bit(eng, pair):
    """5 streams on seeded cuttings of 0, 1, 7, 160, 441, 480 and 4,800-sample pushes, ending at different pushes, one
    slot restarted and reused: the concatenated output of every stream is nhans_resample of its whole input, the
    counts of every push are the contract's, and int16 and float32 input of the same values give the same bits."""
    rng = np.random.default_rng(77 + PAIRS.index(pair))
    lens = [int(rng.integers(3000, 14000)) for _ in range(5)] + [int(rng.integers(900, 6000))]
    lens[1] = 0                                               # a stream that ends without a sample
    xs = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens]
    cuts = [_cut(rng, n) or [0] for n in lens]
    whole = resample.resample(eng, xs, pair[0], pair[1])
    for dtype in (np.int16, np.float32):
        rs = resample.Resampler(eng, 5, pair[0], pair[1], dtype=dtype)
        try:
            data = [x.astype(dtype) for x in xs]
            outs, first = _drive(rs, data[:5], cuts[:5], pair, restart_slot=2, second=data[5], second_cut=cuts[5])
        finally:
            rs.close()
        for i in range(5):
            want = whole[5] if i == 2 else whole[i]
            assert np.array_equal(outs[i], want), (pair, dtype, i)
        assert np.array_equal(first, whole[2])


def test_stream_errors_change_nothing(eng):
    rs = resample.Resampler(eng, 2, 48000, 16000, dtype=np.int16)
    x = np.arange(-500, 500, dtype=np.int16)
    a = rs.push([x[:300], x[:0]], end=[False, True])
    with pytest.raises(hip.NhansError):
        rs.push([x[:0], x[:10]])                              # stream 1 has ended
    with pytest.raises(hip.NhansError):
        rs.restart(2)
    b = rs.push([x[300:], x[:0]], end=[True, False])
    rs.close()
    assert np.array_equal(np.concatenate([a[0], b[0]]), resample.resample(eng, [x], 48000, 16000)[0])
    with pytest.raises(ValueError):
        resample.Resampler(eng, 1, 44100, 48000)
    lib = hip.load()
    off = hip.i64_array([0, 10])
    assert lib.nhans_resample(eng.handle, None, 0, off, 1, 44100, 48000, 0, None, off, None) == -1
    assert b"44100" in lib.nhans_last_error() and b"48000" in lib.nhans_last_error()


def test_peak_normalise_is_apply_normalise(eng):
    """Bit for bit apply.normalise, with the int16 wrap (mono files: |-32768| = -32768) and without (float64 arrays)."""
    rng = np.random.default_rng(5)
    clips = [rng.integers(-3000, 3000, 20000).astype(np.int16),             # several blocks
             np.array([5, -32768, 100, -7], np.int16),
             np.zeros(700, np.int16),
             np.array([-123], np.int16),
             np.full(9, -32768, np.int16),
             np.zeros(0, np.int16),
             rng.integers(-32768, 32768, 8192 + 1).astype(np.int16)]
    clips[0][17000] = -32768
    got = resample.peak_normalise(eng, clips, wrap_int16=True)
    for g, c in zip(got, clips):
        assert np.array_equal(g, apply.normalise(c))
    got = resample.peak_normalise(eng, clips, wrap_int16=False)
    for g, c in zip(got, clips):
        assert np.array_equal(g, apply.normalise(c.astype(np.float64)))
    halves = [c.astype(np.float64) * 0.5 for c in clips]                   # the channel mean of a stereo file
    got = resample.peak_normalise(eng, halves)
    for g, c in zip(got, halves):
        assert np.array_equal(g, apply.normalise(c))


def _recording():
    """1.3 s of 48 kHz int16: a 16 kHz synthetic mixture held for three samples each, plus a tail that fills no hop."""
    x = np.repeat(synth.mixture(901, 1.3), 3)
    return np.ascontiguousarray(x[:len(x) - 101])


def _offline_chain(e, x, ca, cb, peak):
    y = resample.resample(e, [x], 48000, 16000)[0]
    m = apply.trim_to_frames(online.normalise_fixed(y, peak))
    r = e.enhance([m], [ca], [cb], want_mixed=True)
    return [resample.resample(e, [r[k][0]], 16000, 48000)[0] for k in ("denoised_wav", "mixed_wav")]


def _live(e, x, ca, cb, peak):
    enh = online.OnlineEnhancer(e, [ca], [cb], want_mixed=True, in_rate=48000, out_rate=48000, peak=peak)
    den, mix = [], []
    try:
        for i in range(0, len(x), 480):
            (d, m), = enh.push([x[i:i + 480]], end=[i + 480 >= len(x)])
            den.append(d); mix.append(m)
    finally:
        enh.close()
    return np.concatenate(den), np.concatenate(mix)


def test_live_48k_equals_the_offline_chain(eng):
    x = _recording()
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(901))
    peak = 21000
    den, mix = _live(eng, x, ca, cb, peak)
    oden, omix = _offline_chain(eng, x, ca, cb, peak)
    assert len(den) == len(oden) > 48000
    assert np.array_equal(den, oden) and np.array_equal(mix, omix)


def test_without_rates_nothing_is_resampled(eng):
    """Both rates None: the bits of the offline path, and no resample launch in the profile."""
    x = apply.normalise(synth.mixture(902, 1.1))
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(902))
    eng.set_option("profile", 1)
    eng.profile_reset()
    try:
        enh = online.OnlineEnhancer(eng, [ca], [cb], in_rate=None, out_rate=None)
        out = [enh.push([x[i:i + 160]], end=[i + 160 >= len(x)])[0][0] for i in range(0, len(x), 160)]
        enh.close()
        prof = eng.profile()
    finally:
        eng.set_option("profile", 0)
    want = eng.enhance([apply.trim_to_frames(x)], [ca], [cb], want_mixed=False)["denoised_wav"][0]
    assert np.array_equal(np.concatenate(out), want)
    text = str(prof)
    assert "resampl" not in text
    # ... and with rates the launches are counted there
    eng.set_option("profile", 1)
    eng.profile_reset()
    try:
        resample.resample(eng, [np.zeros(100, np.int16)], 48000, 16000)
        assert "resample" in str(eng.profile())
    finally:
        eng.set_option("profile", 0)


def _lite_worker(q):
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        os.environ["NHANS_NO_TORCH"] = "1"
        import nhans_amd  # noqa: F401
        from nhans_amd import lite, weights
        le = lite.LiteEngine("denoiser", weights.synthetic_weights("denoiser", 7))
        x = _recording()
        ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(901))
        den, mix = _live(le, x, ca, cb, 21000)
        oden, omix = _offline_chain(le, x, ca, cb, 21000)
        le.close()
        q.put((den, mix, oden, omix, "torch" in sys.modules, None))
    except Exception as e:
        import traceback
        q.put((None, None, None, None, None, traceback.format_exc() + repr(e)))


def test_live_48k_over_the_torch_free_engine(eng):
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_lite_worker, args=(q,))
    p.start()
    try:
        den, mix, oden, omix, had_torch, err = q.get(timeout=600)
    finally:
        p.join(timeout=120)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert had_torch is False
    assert np.array_equal(den, oden) and np.array_equal(mix, omix)
    x = _recording()
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(901))
    d2, m2 = _live(eng, x, ca, cb, 21000)
    assert np.array_equal(den, d2) and np.array_equal(mix, m2)


def test_argument_errors_change_nothing(eng):
    """Too little room, a negative count, an unknown flag and a bad format are NHANS_EINVAL on the offline call and on the
    push; after each refused push the same push with room succeeds with the bits of the whole."""
    import ctypes
    import torch
    lib = hip.load()
    x = np.arange(-3000, 3000, dtype=np.int16)
    whole = resample.resample(eng, [x], 48000, 16000)[0]
    din = torch.from_numpy(x).to(eng.device)
    dout = torch.zeros(4096, dtype=torch.float32, device=eng.device)
    i64 = hip.i64_array
    no = resample.out_count(len(x), 48000, 16000)
    call = lambda fmt, ioff, flags, ooff: lib.nhans_resample(eng.handle, hip.ptr(din), fmt, i64(ioff), 1, 48000, 16000, flags,
                                                             hip.ptr(dout), i64(ooff), eng._stream())
    assert call(0, [0, len(x)], 0, [0, no - 1]) == -1 and b"room" in lib.nhans_last_error()
    assert call(0, [10, 5], 0, [0, no]) == -1
    assert call(0, [0, len(x)], 2, [0, no]) == -1 and b"flag" in lib.nhans_last_error()
    assert call(7, [0, len(x)], 0, [0, no]) == -1 and b"in_format" in lib.nhans_last_error()
    assert call(0, [0, len(x)], 0, [0, no]) == 0
    assert np.array_equal(dout[:no].cpu().numpy(), whole)
    h = ctypes.c_void_p()
    assert lib.nhans_resampler_open(eng.handle, 1, 48000, 16000, 7, 0, ctypes.byref(h)) == -1
    assert lib.nhans_resampler_open(eng.handle, 1, 48000, 16000, 0, 4, ctypes.byref(h)) == -1
    assert lib.nhans_resampler_open(eng.handle, 0, 48000, 16000, 0, 0, ctypes.byref(h)) == -1
    assert lib.nhans_resampler_open(eng.handle, 1, 48000, 16000, 0, 0, ctypes.byref(h)) == 0
    try:
        got = (ctypes.c_int64 * 1)()
        push = lambda a, b, room, end: lib.nhans_resampler_push(h, ctypes.c_void_p(din.data_ptr() + 2 * a), i64([0, b - a]),
                                                                (ctypes.c_int * 1)(end), hip.ptr(dout), i64([0, room]), got,
                                                                eng._stream())
        outs = []
        assert push(0, 2000, 4096, 0) == 0
        outs.append(dout[:got[0]].cpu().numpy())
        need = resample.emitted(6000, True, 48000, 16000) - resample.emitted(2000, False, 48000, 16000)
        assert push(2000, 6000, need - 1, 1) == -1 and b"room" in lib.nhans_last_error()
        assert lib.nhans_resampler_push(h, hip.ptr(din), i64([5, 0]), None, hip.ptr(dout), i64([0, 4096]), got, eng._stream()) == -1
        assert lib.nhans_resampler_restart(h, 1) == -1 and lib.nhans_resampler_restart(h, -1) == -1
        assert lib.nhans_resampler_set_peak(h, -1.0) == -1
        assert push(2000, 6000, need, 1) == 0 and got[0] == need          # the refused calls changed nothing
        outs.append(dout[:need].cpu().numpy())
        assert np.array_equal(np.concatenate(outs), whole)
        assert push(0, 1, 4096, 0) == -1 and b"ended" in lib.nhans_last_error()
    finally:
        lib.nhans_resampler_close(h)


def test_set_peak_holds_from_the_next_push(eng):
    x = np.random.default_rng(3).integers(-32768, 32768, 4000).astype(np.int16)
    whole = resample.resample(eng, [x], 48000, 16000)[0]
    rs = resample.Resampler(eng, 1, 48000, 16000, dtype=np.int16, peak=1000)
    a, = rs.push([x[:1500]])
    rs.set_peak(30000)
    b, = rs.push([x[1500:]], end=[True])
    rs.close()
    assert np.array_equal(a, online.normalise_fixed(whole[:len(a)], 1000))
    assert np.array_equal(b, online.normalise_fixed(whole[len(a):], 30000))


def test_channel_mean_is_the_float64_mean(eng):
    import torch
    rng = np.random.default_rng(9)
    for C in (1, 2, 3, 6):
        x = rng.integers(-32768, 32768, (C, 1001)).astype(np.float32)
        d = torch.from_numpy(x).to(eng.device).contiguous()
        hip.check(hip.load().nhans_channel_mean(eng.handle, hip.ptr(d), C, 1001, hip.ptr(d), eng._stream()))
        assert np.array_equal(d[0].cpu().numpy(), x.astype(np.float64).mean(axis=0).astype(np.float32))


def _rms(a, b):
    return float(np.sqrt(np.mean(np.square(a.astype(np.float64) - b.astype(np.float64)))))


@pytest.mark.parametrize("mode", ["file", "directory", "online"])
def test_cli_converts_on_the_device(eng, tmp_path, mode):
    """A 44.1 kHz stereo int32 wav and a 48 kHz mono float wav through --convert_on gpu: the denoised file within the
    project's waveform bar (1e-3 RMS) of the --convert_on host run; --output_rate input writes every file at the input's
    rate with ceil(n L / M) samples.  File, directory and --online_ms mode."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    base = synth.mixture(77, 1.6).astype(np.float64)
    x441 = np.clip(0.8 * resample_poly(base, 441, 160), -32000, 32000)
    stereo = np.stack([x441, 0.5 * x441 + 300.0 * np.sin(np.arange(len(x441)) * 0.01)], axis=1)
    inputs = {"a.wav": (44100, np.round(stereo * 65536.0).astype(np.int32)),
              "b.wav": (48000, (resample_poly(base, 3, 1) / 32768.0).astype(np.float32))}
    d = str(tmp_path)
    os.makedirs(os.path.join(d, "in"))
    for name, (rate, data) in inputs.items():
        wavfile.write(os.path.join(d, "in", name), rate, data)
    wavfile.write(os.path.join(d, "neg.wav"), 22050, np.round(resample_poly(synth.noise_context(77).astype(np.float64), 441, 320)).astype(np.int16))
    wavfile.write(os.path.join(d, "pos.wav"), 16000, synth.speaker_context(78, low=False))
    saved = dict(apply._engines)
    apply.set_engine(spec.DENOISER, eng)
    runs = {"host": ["--convert_on", "host"], "gpu": ["--convert_on", "gpu"], "gpu_in": ["--convert_on", "gpu", "--output_rate", "input"]}
    try:
        for tag, extra in runs.items():
            common = ["--neg", os.path.join(d, "neg.wav"), "--pos", os.path.join(d, "pos.wav"), "--weights", "synthetic"] + extra
            if mode == "directory":
                apply.main(["--input", os.path.join(d, "in"), "--output", os.path.join(d, tag)] + common)
            else:
                os.makedirs(os.path.join(d, tag))
                for name in inputs:
                    apply.main(["--input", os.path.join(d, "in", name), "--output", os.path.join(d, tag, name)] + common +
                               (["--online_ms", "10"] if mode == "online" else []))
    finally:
        apply._engines.clear()
        apply._engines.update(saved)
        apply.FLAGS.online_ms = None
        apply.FLAGS.convert_on = "host"
        apply.FLAGS.output_rate = "16000"
    for name, (rate, data) in inputs.items():
        stem = name[:-4]
        for side in ("", "_mixed_processed", "_removed", "_compensated"):
            fn = name if not side else stem + side + ".wav"
            rh, host = wavfile.read(os.path.join(d, "host", fn))
            rg, gpu = wavfile.read(os.path.join(d, "gpu", fn))
            ri, gin = wavfile.read(os.path.join(d, "gpu_in", fn))
            assert rh == rg == 16000 and len(host) == len(gpu) > 16000
            err = _rms(host, gpu)
            print("%s %s%s: RMS(--convert_on gpu, host) = %.3e" % (mode, stem, side, err))
            assert err <= 1e-3
            assert ri == rate and len(gin) == resample.out_count(len(gpu), 16000, rate)
            if not side:
                assert np.array_equal(gin, resample.resample(eng, [gpu], 16000, rate)[0])
