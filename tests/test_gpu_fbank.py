"""Filterbank features on the device (include/nhans_hip.h: nhans_fbank_*; fbank.hip):
  a. float64 parity of fbank_rows over the whole input domain, every element, at the bar of tests/fbank_checks.py;
  b. a row's bits do not depend on where it sits in a call;
  c. online == offline, bit for bit, for three cuttings, two look-aheads and both planes;
  d. nothing else moved: waveforms and launches with and without an attached filterbank;
  e. rewind, restart, detach / attach, slots that computed nothing;
  f. live sessions, mono and split;
  g. the command line.
Small shapes throughout: 53 rows, streams of 0.9 and 1.4 s."""
import json
import os

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import apply, fbank, hip, live, online, resample, spec, synth

import fbank_checks as F

pytestmark = pytest.mark.gpu

PEAK = 21000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    from nhans_amd import engine
    e = engine.Engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    for name in F.BANKS:
        F.bank(name).close()
    e.close()


def _ctx(seed):
    return apply.normalise(synth.silent()), apply.normalise(synth.noise_context(seed))


def _rows(e, fb, rows):
    import torch
    return e.fbank_rows(torch.from_numpy(np.array(rows, dtype=np.float32)).to(e.device), fb).cpu().numpy()


_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _denoised_rows(e):
    """the real denoised rows of one short synthetic clip (48 frames), through the stage-level entry points"""
    def make():
        import torch
        x = apply.trim_to_frames(apply.normalise(synth.mixture(1, 0.5)))
        ca, cb = _ctx(1)
        lm, _ = e.stft_features(torch.from_numpy(np.array(x)).to(e.device), [0, len(x)], want_phase=False)
        cat = torch.from_numpy(np.concatenate([ca, cb])).to(e.device)
        cl, _ = e.stft_features(cat, [0, len(ca), len(ca) + len(cb)], 200, False)
        emb = e.embed(cl.view(2, 200, spec.BINS))
        _, den = e.mask_net(lm, [0, lm.shape[0]], emb[0:1], emb[1:2], want_logits=False)
        return den.cpu().numpy()
    return _once("den", make)


def _batch(e):
    return _once("batch", lambda: np.concatenate([F.uniform_rows(3 * F.TILE + 5), F.edge_rows(), _denoised_rows(e)]))


# ------------------------------------------------------------------------------ a. parity
@pytest.mark.parametrize("name", F.BANKS)
def test_float64_parity_over_the_domain(eng, name):
    """Every element of: 53 uniform rows over [ln 1e-5 - 20, 16], the all-minimum and all-maximum rows, one bin at 16 with
    the rest at the minimum for every bin, and 48 real denoised rows -- one call --, then the uniform rows again in calls
    of 1, tile - 1, tile, tile + 1 and 3 tile + 5 rows.  Bar: C_BAR 2^-24 (K_m + |ref| + 1), tests/fbank_checks.py.
    Measured on an MI355X (profiles/fbank/README.md): worst ratio 2.275 (htk80), 2.545 (slaney128), 2.137 (htk40p1),
    2.257 (custom) -- mostly the device's logf at large |ref| -- hence C_BAR = 8."""
    fb = F.bank(name)
    rows = _batch(eng)
    assert rows[:256].min() == np.float32(F.LO) and rows[:256].max() == np.float32(F.HI)
    got = _rows(eng, fb, rows)
    ref = fb.reference(rows)
    assert got.shape == ref.shape == (rows.shape[0], fb.n_mels) and got.dtype == np.float32
    assert np.all(np.isfinite(got))
    worst = float(F.ratio(fb, got, ref).max())
    uni = rows[:3 * F.TILE + 5]
    for n in (1, F.TILE - 1, F.TILE, F.TILE + 1, 3 * F.TILE + 5):
        g = _rows(eng, fb, uni[:n])
        assert g.shape == (n, fb.n_mels)
        worst = max(worst, float(F.ratio(fb, g, ref[:n]).max()))
        assert np.array_equal(g, got[:n])
    print("fbank parity %s: worst err / (2^-24 (K + |ref| + 1)) = %.3f over %d elements (C_BAR %g)"
          % (name, worst, got.size, F.C_BAR))
    assert F.C_BAR <= 16
    assert worst <= F.C_BAR
    dead = fb.spans()[1] == 0                          # (an empty band: one value, the device's logf(floor), everywhere)
    if dead.any():
        assert np.all(got[:, dead] == got[0, dead][0])
    assert _rows(eng, fb, np.zeros((0, spec.BINS), np.float32)).shape == (0, fb.n_mels)


def test_rows_outside_the_domain(eng):
    """exp(power x) stays a finite float32 whatever the row holds: 2 x = 80 is below the clamp at 88 and every band is at
    the bar; x = 1e30 is clamped, and a single tap of 0.75 gives 88 + ln 0.75; x = -1e30 and -200 give p = 0, ln(floor)."""
    fb = F.bank("custom")
    rows = np.stack([np.full(spec.BINS, v, np.float32) for v in (40.0, 1e30, -1e30, -200.0)])
    got, ref = _rows(eng, fb, rows), fb.reference(rows)
    assert np.all(np.isfinite(got[0])) and np.all(np.abs(got[0] - ref[0]) <= F.bar(fb, ref)[0])
    assert np.isfinite(got[1, 1]) and abs(got[1, 1] - ref[1, 1]) <= F.bar(fb, ref)[1, 1] and ref[1, 1] == 88.0 + np.log(0.75)
    assert not np.any(np.isnan(got))
    assert np.all(got[2:] == got[0, 2]) and abs(got[0, 2] - ref[0, 2]) <= F.bar(fb, ref)[0, 2]      # ln(floor), as the empty band


# ------------------------------------------------------------------------------ b. position independence
@pytest.mark.parametrize("name", ["htk80", "custom"])
def test_bits_do_not_depend_on_the_position(eng, name):
    fb = F.bank(name)
    big = np.array(F.uniform_rows(3 * F.TILE + 5, seed=9))
    five = F.uniform_rows(5, seed=10)
    alone = _rows(eng, fb, five)
    for at in (0, 24, 3 * F.TILE):          # start, across a tile boundary in the middle, the ragged last tile
        b = big.copy()
        b[at:at + 5] = five
        assert np.array_equal(_rows(eng, fb, b)[at:at + 5], alone), at
    assert np.array_equal(np.concatenate([_rows(eng, fb, five[:2]), _rows(eng, fb, five[2:])]), alone)


# ------------------------------------------------------------------------------ c. online == offline
SEC = (0.9, 1.4)
LA = (17, 2)


def _stream(i):
    n = int(SEC[i] * 16000) + 37
    return _once(("x", i), lambda: apply.normalise(synth.mixture(40 + i, SEC[i] + 0.05)[:n]))


def _offline(e, i, name="htk80"):
    """(denoised features, mixed features, denoised wav) of stream i, offline at its look-ahead: made once"""
    def make():
        x = apply.trim_to_frames(_stream(i))
        ca, cb = _ctx(40 + i)
        den, mix = e.features([x], [ca], [cb], F.bank(name), lookahead=LA[i], mixed=True)
        wav = e.enhance([x], [ca], [cb], want_mixed=False, lookahead=LA[i])["denoised_wav"][0]
        return den[0], mix[0], wav
    return _once(("off", i, name), make)


def _cuts(kind):
    lens = [len(_stream(i)) for i in range(2)]
    if kind == "one":
        return [[n] for n in lens]
    if kind == "10ms":
        return [[min(160, n - a) for a in range(0, n, 160)] for n in lens]
    rng = np.random.default_rng(3)
    out = []
    for n in lens:
        c, left = [], n
        while left > 0:
            k = min(left, int(rng.choice([0, 0, 1, 159, 160, 161, 700, 2400])))
            c.append(k)
            left -= k
        out.append(c)
    return out


def _session(e, fb=None, mixed=False):
    s = online.OnlineEnhancer.open_slots(e, 2, lookahead=list(LA))
    for i in range(2):
        s.set_context(i, *_ctx(40 + i))
    if fb is not None:
        s.enable_fbank(fb, mixed=mixed)
    return s


def _drive(s, cuts, planes=(), after_push=None):
    """-> (per stream its concatenated waveform, per plane and stream its concatenated feature rows, pushes that computed
    frames); checks the first-frame numbering on the way"""
    xs = [_stream(i) for i in range(2)]
    pos, wav = [0, 0], [[], []]
    rows = {p: [[], []] for p in planes}
    seen = {p: [0, 0] for p in planes}
    computing = 0
    for k in range(max(len(c) for c in cuts)):
        chunks, end = [], []
        for i in range(2):
            m = cuts[i][k] if k < len(cuts[i]) else 0
            chunks.append(xs[i][pos[i]:pos[i] + m])
            pos[i] += m
            end.append(k == len(cuts[i]) - 1)
        before = [online.ready_frames(s.pushed[i], s.ended[i], LA[i]) for i in range(2)]
        res = s.push(chunks, end)
        after = [online.ready_frames(s.pushed[i], s.ended[i], LA[i]) for i in range(2)]
        computing += any(a > b for a, b in zip(after, before))
        for i in range(2):
            wav[i].append(res[i][0])
            for p in planes:
                first, r = s.features(i, p)
                assert r.shape[0] == after[i] - before[i]
                assert first == before[i] == seen[p][i]
                seen[p][i] += r.shape[0]
                rows[p][i].append(r)
        if after_push is not None:
            after_push(k)
    return ([np.concatenate(w) for w in wav], {p: [np.concatenate(r) for r in rows[p]] for p in planes}, computing)


@pytest.mark.parametrize("kind", ["one", "10ms", "random"])
def test_online_equals_offline(eng, kind):
    """Two streams of 0.9 s (look-ahead 17) and 1.4 s (look-ahead 2) in one object: the rows of all pushes, concatenated,
    are Engine.features of the stream at its look-ahead, the first frames run on from 0 without a gap, the total is T_i;
    plane 1 is fbank_rows of the clip's stft_features rows."""
    import torch
    fb = F.bank("htk80")
    s = _session(eng, fb, mixed=True)
    try:
        wav, rows, _ = _drive(s, _cuts(kind), planes=(0, 1))
    finally:
        s.close()
    for i in range(2):
        den, mix, w = _offline(eng, i)
        T = online.num_frames(len(_stream(i)))
        assert den.shape == mix.shape == (T, 80)
        assert np.array_equal(rows[0][i], den)
        assert np.array_equal(rows[1][i], mix)
        assert np.array_equal(wav[i], w)
        x = apply.trim_to_frames(_stream(i))
        lm, _ = eng.stft_features(torch.from_numpy(np.array(x)).to(eng.device), [0, len(x)], want_phase=False)
        assert np.array_equal(mix, eng.fbank_rows(lm, fb).cpu().numpy())
        assert np.all(np.abs(den - fb.reference(_mask_rows(eng, i))) <= F.bar(fb, fb.reference(_mask_rows(eng, i))))


def _mask_rows(e, i):
    def make():
        import torch
        x = apply.trim_to_frames(_stream(i))
        ca, cb = _ctx(40 + i)
        lm, _ = e.stft_features(torch.from_numpy(np.array(x)).to(e.device), [0, len(x)], want_phase=False)
        cl, _ = e.stft_features(torch.from_numpy(np.concatenate([ca, cb])).to(e.device), [0, len(ca), len(ca) + len(cb)], 200, False)
        emb = e.embed(cl.view(2, 200, spec.BINS))
        e.set_option("lookahead", LA[i])
        try:
            _, den = e.mask_net(lm, [0, lm.shape[0]], emb[0:1], emb[1:2], want_logits=False)
        finally:
            e.set_option("lookahead", spec.LOOKAHEAD)
        return den.cpu().numpy()
    return _once(("mask", i), make)


# ------------------------------------------------------------------------------ d. nothing else moved
def _profiled(e, fb, cuts):
    s = _session(e, fb)
    e.set_option("profile", 1)
    e.profile_reset()
    try:
        wav, _, computing = _drive(s, cuts, planes=(0,) if fb is not None else ())
        prof = {k: v["calls"] for k, v in e.profile().items()}
    finally:
        e.set_option("profile", 0)
        s.close()
    return wav, prof, computing


def test_nothing_else_moved(eng):
    """The same pushes (the random cutting: it has empty pushes and pushes that compute nothing) with and without an
    attached filterbank: bit-identical waveforms; the session that never attaches issues the launches the parent commit
    issued for these pushes (tests/golden/fbank_parent_launches.json, recorded from a build of the parent commit), and
    the attached one exactly one online_fbank more per push that computes frames."""
    cuts = _cuts("random")
    wav_a, prof_a, computing = _profiled(eng, None, cuts)
    wav_b, prof_b, computing_b = _profiled(eng, F.bank("htk80"), cuts)
    for i in range(2):
        assert np.array_equal(wav_a[i], wav_b[i])
    npush = max(len(c) for c in cuts)
    assert 0 < computing == computing_b < npush
    assert "online_fbank" not in prof_a and not any("fbank" in k for k in prof_a)
    assert prof_b.pop("online_fbank") == computing
    assert prof_b == prof_a
    parent = json.load(open(os.path.join(GOLDEN, "fbank_parent_launches.json")))
    assert prof_a == parent


# ------------------------------------------------------------------------------ e. state
def test_rewind_restart_and_reattach(eng):
    fb, fb2 = F.bank("htk80"), F.bank("htk40p1")
    xs = [_stream(0), _stream(1)]
    s = _session(eng, fb)
    try:
        a = [xs[0][:8000], xs[1][:4000]]
        s.push(a, None)
        first0, r0 = s.features(0)
        first1, r1 = s.features(1)
        assert first0 == first1 == 0
        assert r0.shape[0] == online.ready_frames(8000, False, 17) > 0 and r1.shape[0] == online.ready_frames(4000, False, 2) > 0
        assert np.array_equal(r0, _offline(eng, 0)[0][:r0.shape[0]]) and np.array_equal(r1, _offline(eng, 1)[0][:r1.shape[0]])
        with pytest.raises(hip.NhansError):
            s.features(0, plane=1)                      # attached without the mixed plane
        with pytest.raises(hip.NhansError):
            s.features(2)
        # rewind: nothing to read; the repeated push brings the same bits
        s.rewind()
        assert s.features(0)[1].shape == (0, 80) and s.features(1)[1].shape == (0, 80) and s.features(0)[0] == 0
        s.push(a, None)
        assert np.array_equal(s.features(0)[1], r0) and np.array_equal(s.features(1)[1], r1)
        # a push that computes nothing for slot 1 (no samples) and something for slot 0
        s.push([xs[0][8000:8800], xs[1][:0]], None)
        f0, q0 = s.features(0)
        assert f0 == r0.shape[0] and q0.shape[0] == 5
        assert s.features(1)[1].shape[0] == 0 and s.features(1)[0] == r1.shape[0]
        # restart(1): its rows are void and its numbering restarts at 0; slot 0 keeps what the last push computed
        s.push([xs[0][:0], xs[1][4000:4800]], None)
        assert s.features(1)[0] == r1.shape[0] and s.features(1)[1].shape[0] == 5
        s.restart(1)
        assert s.features(1)[1].shape[0] == 0 and s.features(1)[0] == 0
        s.push([xs[0][:0], xs[1][:4000]], None)
        f1, q1 = s.features(1)
        assert f1 == 0 and np.array_equal(q1, r1)
        # detach, then another bank: it applies from the next push on, and the rows of the last one are void
        s.enable_fbank(None)
        with pytest.raises(hip.NhansError):
            s.features(0)
        s.push([xs[0][8800:9600], xs[1][:0]], None)      # frames r0 + 5 .. r0 + 9 get no features
        s.enable_fbank(fb2)
        assert s.features(0)[1].shape == (0, 40)
        s.push([xs[0][9600:10400], xs[1][:0]], None)
        f0, q0 = s.features(0)
        assert f0 == r0.shape[0] + 10 and q0.shape == (5, 40)
        want = eng.features([apply.trim_to_frames(xs[0])], [_ctx(40)[0]], [_ctx(40)[1]], fb2, lookahead=17)[0]
        assert np.array_equal(q0, want[f0:f0 + 5])
    finally:
        s.close()


# ------------------------------------------------------------------------------ f. live
def _recording48(seed):
    return _once(("r48", seed), lambda: np.ascontiguousarray(np.repeat(synth.mixture(seed, 0.8), 3)[:-101].astype(np.int16)))


def _live_offline(e, seed, fb):
    def make():
        y = resample.resample(e, [_recording48(seed)], 48000, 16000)[0]
        m = apply.trim_to_frames(online.normalise_fixed(y, PEAK))
        return e.features([m], [_ctx(seed)[0]], [_ctx(seed)[1]], fb)[0]
    return _once(("lo", seed), make)


def _live_rows(sess, pushes, slots):
    rows = [[] for _ in slots]
    nxt = [0 for _ in slots]
    for chunks, end in pushes:
        sess.push(chunks, end)
        for j, i in enumerate(slots):
            first, r = sess.features(i)
            assert first == nxt[j]
            nxt[j] += r.shape[0]
            rows[j].append(r)
    return [np.concatenate(r) for r in rows]


def test_live_sessions_mono_and_split(eng):
    """48 kHz int16 in pieces of 4,801 samples: the rows are Engine.features of the converted, fixed-peak-normalised
    recording; in a two-channel split session channel c's rows are the mono session's for that channel."""
    fb = F.bank("htk80")
    xs = [_recording48(911), _recording48(912)]
    n = min(len(x) for x in xs)
    xs = [x[:n] for x in xs]
    cuts = [(a, min(a + 4801, n)) for a in range(0, n, 4801)]
    mono = []
    for c in range(2):
        sess = live.LiveSession(eng, 1, 48000, 48000, PEAK)
        try:
            sess.set_context(0, *_ctx(911 + c))
            sess.enable_fbank(fb)
            mono.append(_live_rows(sess, [([xs[c][a:b]], [b == n]) for a, b in cuts], [0])[0])
            with pytest.raises(hip.NhansError) as err:      # (a read returns its rows' count, or the status: one slot)
                sess.features(1)
            assert err.value.code == -1 and "nhans_fbank_live_read: slot 1 outside [0, 1)" in str(err.value)
        finally:
            sess.close()
    for c in range(2):
        assert np.array_equal(mono[c], _live_offline(eng, 911 + c, fb))
    y_frames = online.num_frames(len(resample.resample(eng, [xs[0]], 48000, 16000)[0]))
    assert mono[0].shape == (y_frames, 80) and y_frames > 60
    sess = live.LiveSession(eng, 1, 48000, 48000, PEAK, channels=2, channel_mode="split")
    try:
        for c in sess.slots_of(0):
            sess.set_context(c, *_ctx(911 + c))
        sess.enable_fbank(fb)
        frames = np.ascontiguousarray(np.stack(xs, axis=1))
        split = _live_rows(sess, [([frames[a:b]], [b == n]) for a, b in cuts], sess.slots_of(0))
    finally:
        sess.close()
    for c in range(2):
        assert np.array_equal(split[c], mono[c])


# ------------------------------------------------------------------------------ g. command line
def test_cli_fbank_out(eng, tmp_path):
    from scipy.io import wavfile
    d = str(tmp_path)
    wavfile.write(os.path.join(d, "in.wav"), 16000, synth.mixture(71, 0.5))
    wavfile.write(os.path.join(d, "neg.wav"), 16000, synth.noise_context(71))
    wavfile.write(os.path.join(d, "pos.wav"), 16000, synth.speaker_context(72, low=False))
    saved, flags = dict(apply._engines), dict(vars(apply.FLAGS))
    apply.set_engine("denoiser", eng)
    base = ["--input", os.path.join(d, "in.wav"), "--neg", os.path.join(d, "neg.wav"), "--pos", os.path.join(d, "pos.wav"),
            "--weights", "synthetic"]
    try:
        for tag in ("a", "b"):
            os.mkdir(os.path.join(d, tag))
        apply.main(base + ["--output", os.path.join(d, "a", "denoised.wav")])
        apply.main(base + ["--output", os.path.join(d, "b", "denoised.wav"), "--fbank_out", os.path.join(d, "feats.npy"),
                           "--n_mels", "40", "--mel_scale", "slaney"])
        with pytest.raises(SystemExit):
            apply.main(["--input", d, "--output", d, "--weights", "synthetic", "--fbank_out", os.path.join(d, "x.npy")])
    finally:
        apply._engines.clear()
        apply._engines.update(saved)
        for k in list(vars(apply.FLAGS)):
            if k not in flags:
                delattr(apply.FLAGS, k)
        for k, v in flags.items():
            setattr(apply.FLAGS, k, v)
    names = sorted(os.listdir(os.path.join(d, "a")))
    assert names == sorted(os.listdir(os.path.join(d, "b"))) and len(names) >= 2
    for nme in names:
        assert open(os.path.join(d, "a", nme), "rb").read() == open(os.path.join(d, "b", nme), "rb").read(), nme
    assert sorted(f for f in os.listdir(d) if f.endswith(".npy")) == ["feats.npy"]
    got = np.load(os.path.join(d, "feats.npy"))
    ca, cb, mixed = apply.handle_signals(os.path.join(d, "in.wav"), os.path.join(d, "pos.wav"), os.path.join(d, "neg.wav"))
    fb = fbank.Filterbank(40, scale="slaney")
    try:
        want = eng.features([mixed], [ca], [cb], fb)[0]
    finally:
        fb.close()
    assert got.dtype == np.float32 and got.shape == want.shape == (online.num_frames(len(mixed)), 40)
    assert np.array_equal(got, want)
