"""Online enhancement (nhans_online_*, n-hans_amd/online.py): live recordings pushed piece by piece give exactly the bits
of the offline path (nhans_enhance_clips on the same normalised, trimmed samples), for every push schedule, many streams
in one object, rewind, the saturation fallback, interleaved offline calls, argument errors, the torch-free engine and
the command line."""
import ctypes
import multiprocessing as mp
import os
import warnings

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, online, spec, synth
# (no torch at import time: the torch-free worker below is unpickled from this module in a fresh process)

pytestmark = pytest.mark.gpu

def _engine(*args, **kw):
    from nhans_amd import engine
    return engine.Engine(*args, **kw)


# frames per test stream (the < 400-sample stream is added separately); a 37-sample untrimmed tail on each
FRAMES = [1, 2, 3, 17, 18, 35, 36, 998]
TAIL = 37


def _samples(T):
    return spec.WIN + spec.HOP * (T - 1) + TAIL


def _stream(cid, nsamp):
    x = synth.mixture(cid, nsamp / 16000.0 + 0.01)[:nsamp]
    return apply.normalise(x)


def _ctx(cid):
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


def _run(enh, xs, scheds):
    """Pushes every stream's pieces (streams that are done push nothing); returns the concatenated outputs and checks
    every push's counts against the Python formula and nhans_online_out_counts."""
    S = len(xs)
    pos = [0] * S
    step = [0] * S
    den = [[] for _ in range(S)]
    mix = [[] for _ in range(S)]
    ended = [False] * S
    while not all(ended):
        chunks, end = [], []
        for i in range(S):
            if ended[i]:
                chunks.append(np.zeros(0, np.float32)); end.append(False)
                continue
            k = scheds[i][step[i]]
            step[i] += 1
            chunks.append(xs[i][pos[i]:pos[i] + k])
            end.append(step[i] == len(scheds[i]))
        before = list(enh.pushed)
        want = online.out_counts(before, [len(c) for c in chunks], end, ended)
        assert enh.out_counts([len(c) for c in chunks], end) == want
        outs = enh.push(chunks, end)
        for i in range(S):
            assert len(outs[i][0]) == want[i]
            den[i].append(outs[i][0])
            if outs[i][1] is not None:
                mix[i].append(outs[i][1])
                assert len(outs[i][1]) == want[i]
            pos[i] += len(chunks[i])
            ended[i] = ended[i] or end[i]
            assert online.emitted(enh.pushed[i], ended[i]) == sum(len(d) for d in den[i])
    return [np.concatenate(d) for d in den], [np.concatenate(m) if m else None for m in mix]


@pytest.fixture(scope="module", params=[("denoiser", "f16x3", 1), ("denoiser", "f16x3", 0), ("denoiser", "f32", 1),
                                        ("separator", "f16x3", 1), ("separator", "f32", 1)],
                ids=["den-f16x3-wino", "den-f16x3-direct", "den-f32", "sep-f16x3-wino", "sep-f32"])
def eng(request, lib_built, weights_denoiser, weights_separator):
    kind, prec, wino = request.param
    e = _engine(kind, weights_denoiser if kind == "denoiser" else weights_separator, precision=prec)
    e.set_option("winograd", wino)
    yield e
    e.close()


def test_online_equals_offline_bit_for_bit_for_every_schedule(eng):
    """Streams of 1, 2, 3, 17, 18, 35, 36 and 998 frames plus one of < 400 samples in ONE object, each pushed on its own
    seeded schedule (0- / 1-sample pushes, 399 / 400, whole hops, random pieces), and a second object pushing each clip
    whole with `end`: denoised and mixed output equal the offline run of the trimmed clip, the untrimmed tail ignored."""
    rng = np.random.default_rng(5)
    xs = [_stream(300 + i, _samples(T)) for i, T in enumerate(FRAMES)] + [_stream(399, 250)]
    ctx = [_ctx(300 + i) for i in range(len(xs))]
    ca, cb = [c[0] for c in ctx], [c[1] for c in ctx]
    scheds = [_schedule(rng, len(x)) for x in xs]
    scheds[2] = [160] * (len(xs[2]) // 160) + [len(xs[2]) % 160]          # ends exactly on frame boundaries
    ref = [_offline(eng, xs[i], ca[i], cb[i]) for i in range(len(xs))]
    enh = online.OnlineEnhancer(eng, ca, cb, want_mixed=True)
    den, mix = _run(enh, xs, scheds)
    enh.close()
    whole = online.OnlineEnhancer(eng, ca, cb, want_mixed=True)
    outs = whole.push(xs, end=[True] * len(xs))
    whole.close()
    for i in range(len(xs)):
        assert np.array_equal(den[i], ref[i][0]), i
        assert np.array_equal(mix[i], ref[i][1]), i
        assert np.array_equal(outs[i][0], ref[i][0]), i
        assert np.array_equal(outs[i][1], ref[i][1]), i
    assert len(den[-1]) == 0


def test_six_streams_chunked_push(lib_built, weights_denoiser):
    """S = 6 streams of different lengths ending at different pushes, each equal to its solo offline run; with
    frames_per_chunk = 16 one push runs the stack in several passes."""
    for fpc in (None, 16):
        e = _engine("denoiser", weights_denoiser, precision="f16x3", frames_per_chunk=fpc)
        xs = [_stream(500 + i, _samples(T)) for i, T in enumerate([40, 200, 7, 120, 66, 300])]
        ctx = [_ctx(500 + i) for i in range(6)]
        ca, cb = [c[0] for c in ctx], [c[1] for c in ctx]
        scheds = [[1600 * (i + 1)] * (len(x) // (1600 * (i + 1))) + [len(x) % (1600 * (i + 1))] for i, x in enumerate(xs)]
        enh = online.OnlineEnhancer(e, ca, cb)
        den, mix = _run(enh, xs, scheds)
        enh.close()
        for i in range(6):
            assert mix[i] is None
            assert np.array_equal(den[i], _offline(e, xs[i], ca[i], cb[i])[0]), (fpc, i)
        e.close()


def test_rewind_redo_and_interleaved_calls(lib_built, weights_denoiser):
    """Push X, rewind, push X again: the same bytes and the same later output; one rewind per push; rewind restores an
    ended stream.  Offline enhance calls and a second online object between pushes change nothing."""
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    x = _stream(610, _samples(90))
    ca, cb = _ctx(610)
    ref = _offline(e, x, ca, cb)[0]
    enh = online.OnlineEnhancer(e, [ca], [cb])
    other = online.OnlineEnhancer(e, [cb], [ca], want_mixed=True)
    got = []
    pieces = [4000, 3000, 5000, len(x) - 12000]
    for k, n in enumerate(pieces):
        last = k == len(pieces) - 1
        a = sum(pieces[:k])
        (d1, _), = enh.push([x[a:a + n]], end=[last])
        enh.rewind()
        with pytest.raises(hip.NhansError, match="rewind"):
            enh.rewind()
        assert enh.ended == [False]
        e.enhance([apply.trim_to_frames(_stream(611, 9000))], [ca], [cb])    # offline call in between
        other.push([_stream(612 + k, 2000)])                                 # another object in between
        (d2, _), = enh.push([x[a:a + n]], end=[last])
        assert np.array_equal(d1, d2)
        got.append(d2)
    assert enh.ended == [True]
    enh.rewind()                                                             # the ended stream is open again
    assert enh.ended == [False]
    (d3, _), = enh.push([x[sum(pieces[:-1]):]], end=[True])
    assert np.array_equal(d3, got[-1])
    assert np.array_equal(np.concatenate(got), ref)
    other.close()
    enh.close()
    e.close()


def test_argument_errors_come_back_as_codes(lib_built, weights_denoiser):
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    lib = hip.load()
    ca, cb = _ctx(700)
    enh = online.OnlineEnhancer(e, [ca, ca], [cb, cb])
    enh.push([_stream(700, 1000), np.zeros(0, np.float32)], end=[True, False])
    with pytest.raises(hip.NhansError, match="has ended"):
        enh.push([_stream(700, 10), np.zeros(0, np.float32)])
    with pytest.raises(hip.NhansError, match="has ended"):
        enh.out_counts([5, 0])
    out = (ctypes.c_int64 * 2)()
    rc = lib.nhans_online_push(enh.handle, None, hip.i64_array([0, 0, -2]), None, None, None, hip.i64_array([0, 0, 0]), out, None)
    assert rc == -1 and b"negative" in lib.nhans_last_error()
    rc = lib.nhans_online_push(enh.handle, None, hip.i64_array([0, 0, 5]), None, None, None, hip.i64_array([0, 0, 0]), out, None)
    assert rc == -1 and b"null" in lib.nhans_last_error()
    rc = lib.nhans_online_push(enh.handle, None, None, None, None, None, None, out, None)
    assert rc == -1
    rc = lib.nhans_online_push(None, None, None, None, None, None, None, out, None)
    assert rc == -1
    assert lib.nhans_online_rewind(None) == -1
    enh.close()
    with pytest.raises(hip.NhansError) as ei:
        online.OnlineEnhancer(e, [ca[:32239]], [cb])
    assert "(code -4)" in str(ei.value)                                    # NHANS_ESHORT
    h = ctypes.c_void_p()
    assert lib.nhans_online_open(e.handle, 0, None, None, None, None, 0, None, ctypes.byref(h)) == -1
    assert b"nstreams" in lib.nhans_last_error()
    e.close()


def _scaled_block1(weights_denoiser):           # (as tests/test_gpu_scale.py)
    W = dict(weights_denoiser)
    W["resblock1_1_conv1/w"] = (W["resblock1_1_conv1/w"] * np.float32(3.0e5)).astype(np.float32)
    return W


def test_saturated_push_is_redone_in_f32_and_the_exponents_follow(lib_built, weights_denoiser):
    """Exponents forced to zero on weights that overflow f16: the push warns, its output equals the offline f32 output
    bit for bit, the exponents rise, and the next push runs at f16x3 without the flag."""
    W = _scaled_block1(weights_denoiser)
    x = _stream(7, _samples(60))
    ca, cb = _ctx(7)
    e32 = _engine("denoiser", W, precision="f32")
    ref = _offline(e32, x[:_samples(30) - TAIL], ca, cb)[0]
    e32.close()
    e16 = _engine("denoiser", W, precision="f16x3")
    e16.set_activation_exponents([0] * hip.NUM_ACTIVATIONS)
    enh = online.OnlineEnhancer(e16, [ca], [cb])
    with pytest.warns(UserWarning, match="f16 range"):
        (d, _), = enh.push([x[:_samples(30) - TAIL]], end=[True])
    assert e16.precision == "f16x3"
    assert d.tobytes() == ref.tobytes()                                    # (NaN where the scaled model overflows f32 too)
    assert max(e16.activation_exponents()) >= 10
    enh.close()
    enh = online.OnlineEnhancer(e16, [ca], [cb])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        enh.push([x], end=[True])
    assert e16.take_status() == 0
    enh.close()
    e16.close()


def _lite_worker(q):
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        os.environ["NHANS_NO_TORCH"] = "1"
        import nhans_amd  # noqa: F401
        from nhans_amd import apply, lite, online, synth, weights
        le = lite.LiteEngine("denoiser", weights.synthetic_weights("denoiser", 7))
        x = apply.normalise(synth.mixture(801, 1.3))
        ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(801))
        enh = online.OnlineEnhancer(le, [ca], [cb], want_mixed=True)
        den, mix = [], []
        for i in range(0, len(x), 1234):
            (d, m), = enh.push([x[i:i + 1234]], end=[i + 1234 >= len(x)])
            den.append(d); mix.append(m)
        enh.close()
        le.close()
        q.put((np.concatenate(den), np.concatenate(mix), "torch" in sys.modules, None))
    except Exception as e:
        import traceback
        q.put((None, None, None, traceback.format_exc() + repr(e)))


def test_torch_free_online_equals_the_full_engine(lib_built):
    from nhans_amd import weights
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_lite_worker, args=(q,))
    p.start()
    try:
        den, mix, had_torch, err = q.get(timeout=600)
    finally:
        p.join(timeout=120)
        if p.is_alive():
            p.kill()
    assert err is None, err
    assert had_torch is False
    e = _engine("denoiser", weights.synthetic_weights("denoiser", 7), precision="f16x3")
    x = apply.normalise(synth.mixture(801, 1.3))
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(801))
    enh = online.OnlineEnhancer(e, [ca], [cb], want_mixed=True)
    (d, m), = enh.push([x], end=[True])
    enh.close()
    e.close()
    assert np.array_equal(den, d) and np.array_equal(mix, m)


@pytest.mark.parametrize("prog", ["denoiser", "separator"])
def test_cli_online_writes_the_offline_bytes(lib_built, tmp_path, prog):
    from scipy.io import wavfile
    from nhans_amd import weights
    d = str(tmp_path)
    wavfile.write(os.path.join(d, "in.wav"), 16000, synth.mixture(71, 2.0))
    wavfile.write(os.path.join(d, "neg.wav"), 16000, synth.noise_context(71))
    wavfile.write(os.path.join(d, "pos.wav"), 16000, synth.speaker_context(72, low=False))
    kind = spec.DENOISER if prog == "denoiser" else spec.SEPARATOR
    eng = _engine(kind, weights.synthetic_weights(kind, 7), precision="f16x3")
    main = apply.main if prog == "denoiser" else apply.main_separator
    saved = dict(apply._engines)
    apply.set_engine(kind, eng)
    try:
        for tag, extra in (("off", []), ("on", ["--online_ms", "20"])):
            main(["--input", os.path.join(d, "in.wav"), "--neg", os.path.join(d, "neg.wav"), "--pos", os.path.join(d, "pos.wav"),
                  "--output", os.path.join(d, tag + "denoised.wav"), "--weights", "synthetic"] + extra)
    finally:
        apply._engines.clear()
        apply._engines.update(saved)
        apply.FLAGS.online_ms = None
        eng.close()
    names = ["denoised.wav", "mixed_processed.wav"] + (["removed.wav", "compensated.wav"] if prog == "denoiser" else [])
    for n in names:
        assert open(os.path.join(d, "off" + n), "rb").read() == open(os.path.join(d, "on" + n), "rb").read(), n
