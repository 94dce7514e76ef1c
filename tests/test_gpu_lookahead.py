"""Selectable look-ahead on the device (include/nhans_hip.h: option "lookahead", nhans_online_set_lookahead,
nhans_lookahead_live_set).  den_L -- frame g computed with its clip length taken as min(T, g + L + 1) -- is checked
  1. against the unchanged default path, bit for bit: row g of a ragged default call on the prefixes logmag[:min(T, g+L+1)];
  2. against the float64 oracle on windows whose rows >= T_g are zeroed, at the project's logits bar (1e-4 max-abs on
     identical features, BASELINE.json);
  3. online and live against the offline option, bit for bit, for every cutting and every slot's own L;
  4. set / restart / rewind / mid-stream conditioning / the saturation fallback;
  5. through the command line, with both engines.
Small shapes throughout: 40 - 48 frames."""
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, hip, live, online, resample, spec, synth
from oracle import nhans_oracle as O

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
T40 = 40
TAIL = 37
PEAK = 21000.0


def _engine(*args, **kw):
    from nhans_amd import engine
    return engine.Engine(*args, **kw)


@pytest.fixture(scope="module", params=[("denoiser", "f16x3", 1), ("denoiser", "f16x3", 0), ("denoiser", "f32", 1),
                                        ("separator", "f16x3", 1)],
                ids=["den-f16x3-wino", "den-f16x3-direct", "den-f32", "sep-f16x3-wino"])
def eng(request, lib_built, weights_denoiser, weights_separator):
    kind, prec, wino = request.param
    e = _engine(kind, weights_denoiser if kind == "denoiser" else weights_separator, precision=prec)
    e.set_option("winograd", wino)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_d(lib_built, weights_denoiser):
    e = _engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


def _samples(T):
    return spec.WIN + spec.HOP * (T - 1) + TAIL


def _stream(cid, nsamp):
    return apply.normalise(synth.mixture(cid, nsamp / 16000.0 + 0.01)[:nsamp])


def _ctx(cid):
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(cid))


_feat = {}


def _features(e):
    """(logmag [40, 201], emb_a [1, 512], emb_b [1, 512]) float32 host arrays of one 40-frame clip per model kind: made
    once by the first engine of that kind, then handed unchanged to every engine and to the oracle."""
    import torch
    if e.kind not in _feat:
        x = apply.trim_to_frames(_stream(40, _samples(T40)))
        ca, cb = _ctx(40)
        lm, _ = e.stft_features(torch.from_numpy(x).to(e.device), [0, len(x)])
        cat = torch.from_numpy(np.concatenate([ca, cb])).to(e.device)
        cl, _ = e.stft_features(cat, [0, len(ca), len(ca) + len(cb)], 200, False)
        emb = e.embed(cl.view(2, 200, spec.BINS)).cpu().numpy()
        lm = lm.cpu().numpy()
        assert lm.shape == (T40, spec.BINS)
        for a in (lm, emb):
            a.setflags(write=False)
        _feat[e.kind] = (lm, emb[0:1], emb[1:2])
    return _feat[e.kind]


def _mask_net(e, lm, foff, ea, eb, nclips=1):
    import torch
    d = e.device
    lg, den = e.mask_net(torch.from_numpy(np.array(lm, dtype=np.float32)).to(d), foff,
                         torch.from_numpy(np.repeat(ea, nclips, 0)).to(d), torch.from_numpy(np.repeat(eb, nclips, 0)).to(d))
    return lg.cpu().numpy(), den.cpu().numpy()


# ------------------------------------------------------------------------------ 1. offline option == default path
@pytest.mark.parametrize("L", [0, 3])
def test_option_equals_the_default_path_on_prefix_clips(eng, L):
    """One call with option L on the 40-frame clip against ONE ragged call at the default option whose clip g is the
    prefix logmag[:min(T, g + L + 1)]: row g of clip g, logits and denoised, bit for bit -- frame g of the option call
    must read exactly what the last-but-L-th frame of a clip that really ends there reads."""
    lm, ea, eb = _features(eng)
    eng.set_option("lookahead", L)
    try:
        lg_L, den_L = _mask_net(eng, lm, [0, T40], ea, eb)
    finally:
        eng.set_option("lookahead", 17)
    lens = [min(T40, g + L + 1) for g in range(T40)]
    foff = [0]
    for n in lens:
        foff.append(foff[-1] + n)
    lg_p, den_p = _mask_net(eng, np.concatenate([lm[:n] for n in lens]), foff, ea, eb, nclips=T40)
    rows = [foff[g] + g for g in range(T40)]
    assert np.array_equal(lg_L, lg_p[rows]) and np.array_equal(den_L, den_p[rows])
    lg_17, _ = _mask_net(eng, lm, [0, T40], ea, eb)
    assert np.array_equal(lg_17[T40 - 1 - L:], lg_L[T40 - 1 - L:])       # the last L + 1 frames see the real end either way
    assert not np.array_equal(lg_17[:T40 - 1 - L], lg_L[:T40 - 1 - L])


def test_option_range_and_default(eng):
    lib = hip.load()
    for bad in (-1, 18):
        assert lib.nhans_set_option(eng.handle, b"lookahead", bad) == -1 and b"lookahead" in lib.nhans_last_error()
    lm, ea, eb = _features(eng)
    ref = _mask_net(eng, lm, [0, T40], ea, eb)[0]
    eng.set_option("lookahead", 17)
    assert np.array_equal(_mask_net(eng, lm, [0, T40], ea, eb)[0], ref)


# ------------------------------------------------------------------------------ 2. against float64
_oracle = {}


def _oracle_logits(kind, W, L, frames):
    key = (kind, L)
    if key not in _oracle:
        lm, ea, eb = _feat[kind]
        win = O.strided_crop(lm.astype(np.float64), spec.MIX_WIN)[frames].copy()
        for k, g in enumerate(frames):
            Tg = min(T40, g + L + 1)
            for h in range(spec.MIX_WIN):
                if g + h - spec.CENTER >= Tg:
                    win[k, h] = 0.0
        n = len(frames)
        out, den = O.mask_net(win, np.repeat(ea, n, 0).astype(np.float64), np.repeat(eb, n, 0).astype(np.float64), W, kind)
        _oracle[key] = (out, den)
    return _oracle[key]


@pytest.mark.parametrize("L", [0, 2])
def test_option_against_the_float64_oracle(eng, L, weights_denoiser, weights_separator):
    lm, ea, eb = _features(eng)
    frames = [0, 5, T40 - 1 - L, T40 - 1]
    W = weights_denoiser if eng.kind == "denoiser" else weights_separator
    ref_lg, ref_den = _oracle_logits(eng.kind, W, L, frames)
    eng.set_option("lookahead", L)
    try:
        lg, den = _mask_net(eng, lm, [0, T40], ea, eb)
    finally:
        eng.set_option("lookahead", 17)
    err = np.abs(lg[frames] - ref_lg).max(axis=1)
    print("L = %d, %s %s: max |logit - float64| on frames %s = %s" % (L, eng.kind, eng.precision, frames, err))
    assert err.max() < LOGIT_TOL
    assert np.abs(den[frames] - ref_den).max() < LOGIT_TOL


# ------------------------------------------------------------------------------ 3. online / live == offline den_L
LS = [0, 1, 2, 16, 17]
T_ON = 48


def _offline(e, x, ca, cb, L):
    m = apply.trim_to_frames(x)
    if len(m) < spec.WIN:
        return np.zeros(0, np.float32), np.zeros(0, np.float32)
    r = e.enhance([m], [ca], [cb], want_mixed=True, lookahead=L)
    return r["denoised_wav"][0], r["mixed_wav"][0]


def _schedules(rng, n):
    """Five cuttings of n samples: everything in one push; everything, then an end flag with 0 samples; 1-sample pushes
    across the first frame's completion and the first hop after it; two seeded mixtures of 0 / 1 / 399 / 400 / hop /
    random pieces."""
    def seeded():
        out, left = [], n
        while left > 0:
            k = min(int(rng.choice([0, 1, 399, 400, 160, 320, int(rng.integers(1, 3000))])), left)
            out.append(k)
            left -= k
        return out
    ones = [390] + [1] * 180 + [n - 570]
    return [[n], [n, 0], ones, seeded(), seeded()]


def _run(enh, xs, scheds):
    """As tests/test_gpu_online.py: pushes every stream's pieces, checks every push's counts against the Python formula
    with the slot's L and against nhans_online_out_counts."""
    S = len(xs)
    pos, step, ended = [0] * S, [0] * S, [False] * S
    den, mix = [[] for _ in range(S)], [[] for _ in range(S)]
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
        want = online.out_counts(list(enh.pushed), [len(c) for c in chunks], end, ended, lookahead=enh.lookahead)
        assert enh.out_counts([len(c) for c in chunks], end) == want
        outs = enh.push(chunks, end)
        for i in range(S):
            assert len(outs[i][0]) == len(outs[i][1]) == want[i]
            den[i].append(outs[i][0]); mix[i].append(outs[i][1])
            pos[i] += len(chunks[i])
            ended[i] = ended[i] or end[i]
            assert online.emitted(enh.pushed[i], ended[i], enh.lookahead[i]) == sum(len(d) for d in den[i])
    return [np.concatenate(d) for d in den], [np.concatenate(m) for m in mix]


def test_online_equals_offline_for_every_cutting_and_lookahead(eng):
    """One object, slots at L = 0, 1, 2, 16, 17 on the same 48-frame recording, a stream of 2 frames at L = 2 (shorter
    than L + 1) and one of 250 samples (0 frames); run twice with the five cuttings rotated over the slots.  Denoised
    and mixed output of every slot equal the offline call with option L, bit for bit."""
    x = _stream(900, _samples(T_ON))
    short, none = _stream(901, _samples(2)), _stream(902, 250)
    ca, cb = _ctx(900)
    ref = {L: _offline(eng, x, ca, cb, L) for L in LS}
    ref_short = _offline(eng, short, ca, cb, 2)
    assert len(ref_short[0]) == 560 and not np.array_equal(ref[2][0], ref[17][0])
    assert np.array_equal(ref[0][1], ref[17][1])                 # (the mixed round trip does not depend on L)
    xs = [x] * 5 + [short, none]
    las = LS + [2, 2]
    rng = np.random.default_rng(17)
    for turn in (0, 3):
        sch = _schedules(rng, len(x))
        scheds = [sch[(i + turn) % 5] for i in range(5)] + [[len(short)], [100, 150]]
        enh = online.OnlineEnhancer(eng, [ca] * 7, [cb] * 7, want_mixed=True, lookahead=las)
        try:
            assert enh.lookahead == las
            den, mix = _run(enh, xs, scheds)
        finally:
            enh.close()
        for i, L in enumerate(LS):
            assert np.array_equal(den[i], ref[L][0]), (turn, L)
            assert np.array_equal(mix[i], ref[L][1]), (turn, L)
        assert np.array_equal(den[5], ref_short[0]) and np.array_equal(mix[5], ref_short[1])
        assert len(den[6]) == 0 and len(mix[6]) == 0


def _recording48(seed):
    """0.5 s (48 frames at 16 kHz) of int16 at 48 kHz with a tail that fills no hop."""
    return np.ascontiguousarray(np.repeat(synth.mixture(seed, 0.5), 3)[:-101].astype(np.int16))


def _live_reference(e, x48, ca, cb, L, wet, scale):
    y = resample.resample(e, [x48], 48000, 16000)[0]
    m = apply.trim_to_frames(online.normalise_fixed(y, PEAK))
    r = e.enhance([m], [ca], [cb], want_mixed=True, lookahead=L)
    den, mix = r["denoised_wav"][0], r["mixed_wav"][0]
    c = den + (mix - den) * np.float32(wet)
    v = (resample.resample(e, [c], 16000, 48000)[0].astype(np.float64) * scale).astype(np.float32)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("wet", [0.0, 0.25])
def test_live_session_48k_int16_equals_the_offline_chain(eng, wet):
    """LiveSession 48 kHz int16 both ways, slots at L = 0, 2 and 17, 10 ms pieces / one push / a seeded cutting: bit for
    bit resample -> normalise -> trim -> enhance(lookahead=L) -> wet mix -> resample -> scale -> round."""
    x = _recording48(903)
    ca, cb = _ctx(903)
    las = [0, 2, 17]
    scale = live.default_out_scale(PEAK, np.int16)
    want = [_live_reference(eng, x, ca, cb, L, wet, scale) for L in las]
    rng = np.random.default_rng(4)
    seeded, left = [], len(x)
    while left > 0:
        k = min(int(rng.choice([0, 1, 7, 441, 480, 4800])), left)
        seeded.append(k); left -= k
    cuts = [[480] * (len(x) // 480) + [len(x) % 480], [len(x), 0], seeded]
    sess = live.LiveSession(eng, 3, 48000, 48000, PEAK, wet=wet != 0, lookahead=las)
    try:
        for i in range(3):
            sess.set_context(i, ca, cb)
        sess.set_wet(wet)
        got = [[] for _ in las]
        pos, step = [0] * 3, [0] * 3
        while any(step[i] < len(cuts[i]) for i in range(3)):
            chunks, end = [], []
            for i in range(3):
                k = cuts[i][step[i]] if step[i] < len(cuts[i]) else 0
                chunks.append(x[pos[i]:pos[i] + k])
                pos[i] += k
                step[i] += step[i] < len(cuts[i])
                end.append(step[i] == len(cuts[i]) and not sess.ended[i])
            cnt = [live.emitted(sess.pushed[i] + len(chunks[i]), bool(end[i] or sess.ended[i]), 48000, 48000, las[i])
                   - live.emitted(sess.pushed[i], sess.ended[i], 48000, 48000, las[i]) for i in range(3)]
            assert sess.out_counts([len(c) for c in chunks], end) == cnt
            for i, o in enumerate(sess.push(chunks, end)):
                assert len(o) == cnt[i]
                got[i].append(o)
    finally:
        sess.close()
    for i, L in enumerate(las):
        g = np.concatenate(got[i])
        assert g.dtype == np.int16 and np.array_equal(g, want[i]), (L, wet)
    assert not np.array_equal(want[0], want[2])


# ------------------------------------------------------------------------------ 4. further checks
def test_lookahead_17_set_explicitly_gives_the_default_bits(eng):
    x = _stream(910, _samples(T40))
    ca, cb = _ctx(910)
    outs = []
    for la in (None, 17):
        kw = {} if la is None else {"lookahead": la}
        enh = online.OnlineEnhancer(eng, [ca], [cb], want_mixed=True, **kw)
        if la is not None:
            enh.set_lookahead(0, 17)
            eng.set_option("lookahead", 17)
        d = [enh.push([x[a:a + 2500]], end=[a + 2500 >= len(x)])[0] for a in range(0, len(x), 2500)]
        enh.close()
        outs.append((np.concatenate([p[0] for p in d]), np.concatenate([p[1] for p in d])))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    off = eng.enhance([apply.trim_to_frames(x)], [ca], [cb], want_mixed=True)
    assert np.array_equal(outs[0][0], off["denoised_wav"][0])
    assert np.array_equal(_offline(eng, x, ca, cb, 17)[0], off["denoised_wav"][0])


def test_the_context_option_does_not_reach_online_objects(eng):
    """Online objects carry their own L: the context's option at 3 changes nothing for a slot at 2 or at 17."""
    x = _stream(911, _samples(T40))
    ca, cb = _ctx(911)
    ref = {L: _offline(eng, x, ca, cb, L)[0] for L in (2, 17)}
    eng.set_option("lookahead", 3)
    try:
        enh = online.OnlineEnhancer(eng, [ca, ca], [cb, cb], lookahead=[2, 17])
        outs = enh.push([x, x], end=[True, True])
        enh.close()
    finally:
        eng.set_option("lookahead", 17)
    assert np.array_equal(outs[0][0], ref[2]) and np.array_equal(outs[1][0], ref[17])


def test_set_lookahead_rules_restart_and_rewind(eng_d):
    """EINVAL on a stream with samples or an ended one, counts untouched; L survives restart; the call makes the last push
    final; rewind + redo at L = 2 give the same bits and the stream still ends on the offline output."""
    e, lib = eng_d, hip.load()
    x = _stream(912, _samples(T40))
    ca, cb = _ctx(912)
    ref = _offline(e, x, ca, cb, 2)[0]
    enh = online.OnlineEnhancer(e, [ca, ca], [cb, cb], lookahead=[2, 17])
    (d1, _), _ = enh.push([x[:3000], x[:0]])
    assert len(d1) == online.emitted(3000, False, 2) == 160 * 14
    counts = enh.out_counts([1000, 1000])
    for L in (0, 2, 17):
        assert lib.nhans_online_set_lookahead(enh.handle, 0, L) == -1 and b"under way" in lib.nhans_last_error()
    assert lib.nhans_online_set_lookahead(enh.handle, 1, 18) == -1 and lib.nhans_online_set_lookahead(enh.handle, 2, 2) == -1
    with pytest.raises(hip.NhansError, match="under way"):
        enh.set_lookahead(0, 5)
    assert enh.lookahead == [2, 17] and enh.out_counts([1000, 1000]) == counts
    enh.rewind()                                                        # (the refused calls left the push undoable)
    (d2, _), _ = enh.push([x[:3000], x[:0]])
    assert np.array_equal(d1, d2)
    enh.set_lookahead(1, 4)                                             # slot 1 has no samples yet: allowed ...
    with pytest.raises(hip.NhansError, match="rewind"):                 # ... and it makes the last push final
        enh.rewind()
    (d3, _), (s1, _) = enh.push([x[3000:], x], end=[True, True])
    assert np.array_equal(np.concatenate([d2, d3]), ref)
    assert np.array_equal(s1, _offline(e, x, ca, cb, 4)[0])
    assert lib.nhans_online_set_lookahead(enh.handle, 0, 2) == -1       # ended
    enh.restart(0)
    assert enh.out_counts([3000, 0]) == [160 * 14, 0]                   # L = 2 survived the restart
    (d4, _), _ = enh.push([x, x[:0]], end=[True, False])
    assert np.array_equal(d4, ref)
    enh.close()


def test_live_set_lookahead_rules_and_rewind(eng_d):
    e, lib = eng_d, hip.load()
    x = _recording48(913)
    ca, cb = _ctx(913)
    want = _live_reference(e, x, ca, cb, 2, 0.0, live.default_out_scale(PEAK, np.int16))
    sess = live.LiveSession(e, 1, 48000, 48000, PEAK)
    sess.set_context(0, ca, cb)
    sess.set_lookahead(0, 2)
    a = sess.push([x[:9000]])[0]
    assert len(a) == live.emitted(9000, False, 48000, 48000, 2) > live.emitted(9000, False, 48000, 48000) == 0
    counts = sess.out_counts([4800])
    assert lib.nhans_lookahead_live_set(sess.handle, 0, 0) == -1 and b"under way" in lib.nhans_last_error()
    assert lib.nhans_lookahead_live_set(sess.handle, 0, 18) == -1 and lib.nhans_lookahead_live_set(sess.handle, 1, 2) == -1
    assert sess.out_counts([4800]) == counts
    sess.rewind()
    a2 = sess.push([x[:9000]])[0]
    b = sess.push([x[9000:]], end=[True])[0]
    assert np.array_equal(a, a2) and np.array_equal(np.concatenate([a2, b]), want)
    sess.restart(0)
    assert sess.out_counts([9000]) == [len(a)]                          # L = 2 survived the restart
    sess.set_lookahead(0, 17)
    assert sess.out_counts([9000]) == [0]
    sess.close()


def test_conditioning_change_mid_stream_at_lookahead_2(eng_d):
    """set_context on a running stream at L = 2 reports R = T - 2 and obeys change_bounds(R) against the two offline
    outputs of option L = 2."""
    e = eng_d
    x = _stream(914, _samples(T40))
    ca, cb = _ctx(914)
    ca2, cb2 = _ctx(915)[1], _ctx(916)[1]
    den1, mix1 = _offline(e, x, ca, cb, 2)
    den2, _ = _offline(e, x, ca2, cb2, 2)
    n1 = spec.WIN + spec.HOP * 20 + 5                                   # 21 frames pushed: R = 19 at L = 2 (2 at L = 17)
    enh = online.OnlineEnhancer(e, [ca], [cb], want_mixed=True, lookahead=2)
    (a, ma), = enh.push([x[:n1]])
    R = enh.set_context(0, ca2, cb2)
    assert R == 19 == enh.first_new_frame(0) == online.ready_frames(n1, False, 2)
    (b, mb), = enh.push([x[n1:]], end=[True])
    enh.close()
    got, lo_hi = np.concatenate([a, b]), online.change_bounds(R)
    assert lo_hi == (160 * 18, 160 * 20 + 240)
    assert np.array_equal(got[:lo_hi[0]], den1[:lo_hi[0]]) and np.array_equal(got[lo_hi[1]:], den2[lo_hi[1]:])
    assert np.isfinite(got).all() and not np.array_equal(den1[lo_hi[1]:], den2[lo_hi[1]:])
    assert np.array_equal(np.concatenate([ma, mb]), mix1)


def _scaled_block1(weights_denoiser):           # (as tests/test_gpu_online.py)
    W = dict(weights_denoiser)
    W["resblock1_1_conv1/w"] = (W["resblock1_1_conv1/w"] * np.float32(3.0e5)).astype(np.float32)
    return W


def test_saturated_fallbacks_keep_the_lookahead(lib_built, weights_denoiser):
    """Exponents forced to zero on weights that overflow f16: the online push and the offline call at L = 2 both warn and
    come back with the bits of the f32 engine at L = 2."""
    W = _scaled_block1(weights_denoiser)
    x = apply.trim_to_frames(_stream(7, _samples(30)))
    ca, cb = _ctx(7)
    e32 = _engine("denoiser", W, precision="f32")
    ref = {L: e32.enhance([x], [ca], [cb], lookahead=L)["denoised_wav"][0] for L in (2, 17)}
    e32.close()
    assert ref[2].tobytes() != ref[17].tobytes()
    e16 = _engine("denoiser", W, precision="f16x3")
    e16.set_activation_exponents([0] * hip.NUM_ACTIVATIONS)
    enh = online.OnlineEnhancer(e16, [ca], [cb], lookahead=2)
    with pytest.warns(UserWarning, match="f16 range"):
        (d, _), = enh.push([x], end=[True])
    enh.close()
    assert e16.precision == "f16x3" and d.tobytes() == ref[2].tobytes()
    e16.set_activation_exponents([0] * hip.NUM_ACTIVATIONS)
    with pytest.warns(UserWarning, match="f16 range"):
        off = e16.enhance([x], [ca], [cb], lookahead=2)["denoised_wav"][0]
    assert off.tobytes() == ref[2].tobytes()
    e16.close()


# ------------------------------------------------------------------------------ 5. command line
@pytest.mark.parametrize("which", ["engine", "lite"])
def test_cli_lookahead_file_mode_equals_online_mode(lib_built, tmp_path, weights_denoiser, which):
    from scipy.io import wavfile
    d = str(tmp_path)
    wavfile.write(os.path.join(d, "in.wav"), 16000, synth.mixture(71, 0.5))
    wavfile.write(os.path.join(d, "neg.wav"), 16000, synth.noise_context(71))
    wavfile.write(os.path.join(d, "pos.wav"), 16000, synth.speaker_context(72, low=False))
    if which == "engine":
        e = _engine("denoiser", weights_denoiser, precision="f16x3")
    else:
        from nhans_amd import lite
        e = lite.LiteEngine("denoiser", weights_denoiser)
    saved, flags = dict(apply._engines), dict(vars(apply.FLAGS))
    apply.set_engine("denoiser", e)
    try:
        for tag, extra in (("def", []), ("off", ["--lookahead_ms", "20"]), ("on", ["--lookahead_ms", "20", "--online_ms", "10"])):
            apply.main(["--input", os.path.join(d, "in.wav"), "--neg", os.path.join(d, "neg.wav"), "--pos", os.path.join(d, "pos.wav"),
                        "--output", os.path.join(d, tag + "denoised.wav"), "--weights", "synthetic"] + extra)
    finally:
        apply._engines.clear()
        apply._engines.update(saved)
        for k in list(vars(apply.FLAGS)):
            if k not in flags:
                delattr(apply.FLAGS, k)
        for k, v in flags.items():
            setattr(apply.FLAGS, k, v)
        e.close()
    rd = lambda n: open(os.path.join(d, n), "rb").read()
    for n in ("denoised.wav", "mixed_processed.wav", "removed.wav", "compensated.wav"):
        assert rd("off" + n) == rd("on" + n), n
    assert rd("offdenoised.wav") != rd("defdenoised.wav")
    assert rd("offmixed_processed.wav") == rd("defmixed_processed.wav")
