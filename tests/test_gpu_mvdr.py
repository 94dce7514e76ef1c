"""Mask-driven MVDR beamforming on the device (mvdr.hip, nhans_mvdr_*) against the float64 definition nhans_amd.mvdr,
teacher-forced stage by stage within the bars of tests/mvdr_checks.py: spectra, covariances, weights, filter and rows and
the records on every shape; the bits' independence of batch, position, run and call path; the edge inputs; the memory
contract and the refusals; enhance_array against the composition of the public calls; and apply.array_ceiling on the
simulated scenes against float64.  Every test prints its figures (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import apply, context, engine, hip, mvdr, spec, synth

from oracle import nhans_oracle as O

import mvdr_checks as M

pytestmark = pytest.mark.gpu

BINS = mvdr.BINS
TAILS = (0, 159, 1, 80, 37, 0, 0)               # untrimmed samples behind the last frame of the clips of COUNTS


@pytest.fixture(scope="module")
def eng(weights_denoiser, lib_built):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same(a, b, keys=("logmag", "phase", "w")):
    return all(bits(a[k]) == bits(b[k]) for k in keys) and bits(np.array(list(a["record"].values()))) == bits(np.array(list(b["record"].values())))


def shape_batch(C, loggain):
    clips = [M.random_clip(T, C, 7000 + 10 * C + i, tail) for i, (T, tail) in enumerate(zip(M.COUNTS, TAILS))]
    masks = [M.random_mask(T, 7100 + 10 * C + i, loggain) for i, T in enumerate(M.COUNTS)]
    return clips, masks


@pytest.mark.parametrize("C", [1, 2, 3, 8])
@pytest.mark.parametrize("variant", ["mask rows, last channel, default loading", "log-gain rows, channel 0, no loading"])
def test_every_stage_on_every_shape(eng, C, variant):
    """T = 1, 2, 3, 63, 64, 65, 138 in one ragged batch (five clips with untrimmed tails) through the three stage calls;
    every stage against the definition on the device's own output of the stage before."""
    loggain = variant.startswith("log-gain")
    ref, loading = (0, 0.0) if loggain else (C - 1, mvdr.LOADING)
    clips, masks = shape_batch(C, loggain)
    got = eng.mvdr(clips, masks, ref=ref, loading=loading, loggain=loggain, stages=True)
    # the row invariant: the analysis rows of every channel are nhans_stft_features' of the planes as clips of their own
    pf = np.concatenate([mvdr.planes(x) for x in clips])
    off = context.offsets(len(x) for x in clips for _ in range(C))
    lm_t, ph_t = eng.stft_features(torch.from_numpy(pf).cuda(), off)
    assert bits(np.concatenate([g["chan_logmag"].reshape(-1, BINS) for g in got])) == bits(lm_t.cpu().numpy())
    assert bits(np.concatenate([g["chan_phase"].reshape(-1, BINS) for g in got])) == bits(ph_t.cpu().numpy())
    ratio = M.spectrum_ratio(("shapes", C), [x[:, c] for x in clips for c in range(C)])
    worst = dict(spectra=0.0, cov=0.0, w=0.0, y=0.0, lm=0.0, ph=0.0)
    left_out = 0
    for i, (x, m, g) in enumerate(zip(clips, masks, got)):
        T = M.COUNTS[i]
        label = "C %d T %d" % (C, T)
        n = spec.WIN + spec.HOP * (T - 1)
        v = M.check_spectra(label, g["X"], x[:n], ratio)
        assert v.ok, v.message
        worst["spectra"] = max(worst["spectra"], v.rel)
        v = M.check_covariances(label, g["phi_s"], g["phi_n"], g["X"], mvdr.mask_values(m, loggain), mask_rel=M.EXP_REL if loggain else 0.0)
        assert v.ok, v.message
        worst["cov"] = max(worst["cov"], v.rel)
        v = M.check_weights(label, g["w"], g["phi_s"], g["phi_n"], ref, loading)
        assert v.ok, v.message
        worst["w"] = max(worst["w"], v.rel)
        left_out += int((~v.judged).sum())
        v = M.check_filter(label, g["y"], g["logmag"], g["phase"], g["X"], g["w"])
        assert v.ok, v.message
        worst["y"], worst["lm"], worst["ph"] = max(worst["y"], v.rel), max(worst["lm"], v.rel_lm), max(worst["ph"], v.rel_ph)
        rec = g["record"]
        e_ref, e_out, tol = M.record_bars(rec, g["X"], g["y"], ref)
        assert (rec["frames"], rec["channels"], rec["ref"]) == (T, C, ref)
        if C > 1:       # the record against the device's own w (self-consistency; against the definition: check_weights, the edge test)
            assert rec["fallback_bins"] == int(np.all(g["w"] == np.eye(C)[ref][None, :], axis=1).sum()), label
        assert abs(rec["energy_ref"] - e_ref) <= tol * e_ref and abs(rec["energy_out"] - e_out) <= tol * e_out, (label, rec, e_ref, e_out)
    print("C %d, %s: measured / bar -- spectra %.3f, covariances %.3f, weights %.3f, y %.3f, lm %.3f, ph %.3f; bins left out as "
          "ill-conditioned: %d of %d" % (C, variant, worst["spectra"], worst["cov"], worst["w"], worst["y"], worst["lm"], worst["ph"],
                                         left_out, BINS * len(clips)))


def test_gain_is_added_in_the_filter_launch(eng):
    x, m = M.random_clip(40, 3, 7301), M.random_mask(40, 7302)
    gain = np.random.default_rng(7303).uniform(-3.0, 0.5, (40, BINS)).astype(np.float32)
    plain = eng.mvdr([x], [m], stages=True)[0]
    for stages in (False, True):
        g = eng.mvdr([x], [m], gains=[gain], stages=stages)[0]
        assert bits(g["logmag"]) == bits(plain["logmag"] + gain) and bits(g["phase"]) == bits(plain["phase"])
        assert g["record"] == plain["record"]


@pytest.mark.parametrize("C", [2, 8])
def test_bits_alone_batched_moved_again_and_by_either_path(eng, C):
    clips, masks = shape_batch(C, False)
    batch = eng.mvdr(clips, masks, ref=1)
    again = eng.mvdr(clips, masks, ref=1)
    staged = eng.mvdr(clips, masks, ref=1, stages=True)
    order = list(range(len(clips)))[::-1]
    moved = eng.mvdr([clips[i] for i in order], [masks[i] for i in order], ref=1)
    for i in range(len(clips)):
        alone = eng.mvdr([clips[i]], [masks[i]], ref=1)[0]
        for other in (batch[i], again[i], staged[i], moved[order.index(i)]):
            assert same(alone, other), "clip %d" % i
        assert np.isfinite(alone["logmag"]).all() and np.isfinite(alone["w"]).all()


def test_edge_inputs_fall_back_as_the_definition_says(eng):
    T = 12
    n = spec.WIN + spec.HOP * (T - 1)
    half = np.full((T, BINS), 0.5, np.float32)
    silent = np.zeros((n, 3), np.float32)
    dead = M.random_clip(T, 3, 7401); dead[:, 1] = 0.0
    twin = np.repeat(M.random_clip(T, 1, 7402), 3, axis=1)
    one8 = M.random_clip(1, 8, 7403)
    ones = M.random_clip(T, 3, 7404)
    cases = [("a silent clip", silent, half, mvdr.LOADING, BINS), ("an all-zero channel", dead, M.random_mask(T, 7405), mvdr.LOADING, None),
             ("an all-zero channel, no loading", dead, M.random_mask(T, 7405), 0.0, BINS),
             ("identical channels", twin, M.random_mask(T, 7406), mvdr.LOADING, None),
             ("one frame, eight channels", one8, np.full((1, BINS), 0.5, np.float32), mvdr.LOADING, None),
             ("a mask of ones", ones, np.ones((T, BINS), np.float32), mvdr.LOADING, BINS),
             ("a mask of zeros", ones, np.zeros((T, BINS), np.float32), mvdr.LOADING, BINS),
             ("a mask of NaN", ones, np.full((T, BINS), np.nan, np.float32), mvdr.LOADING, BINS)]
    for name, x, m, loading, want in cases:
        g = eng.mvdr([x], [m], loading=loading, stages=True)[0]
        r = mvdr.reference(x, m, loading=loading, X=g["X"])
        for k in ("logmag", "phase", "w", "y", "phi_s", "phi_n"):
            assert np.isfinite(g[k]).all(), (name, k)
        assert np.isfinite(list(g["record"].values())).all(), name
        print("%-34s fallback bins: device %3d, definition %3d" % (name, g["record"]["fallback_bins"], r["record"]["fallback_bins"]))
        assert g["record"]["fallback_bins"] == r["record"]["fallback_bins"], name
        if want is not None:
            assert g["record"]["fallback_bins"] == want, name
        if want == BINS:                                # the reference channel passes through, value for value
            assert np.array_equal(g["y"], g["X"][0]), name
            e_ref, e_out, tol = M.record_bars(g["record"], g["X"], g["y"], 0)     # (the two energies are summed in two orders)
            assert abs(g["record"]["energy_out"] - e_out) <= tol * e_out and abs(g["record"]["energy_ref"] - e_ref) <= tol * e_ref, name
        v = M.check_weights(name, g["w"], g["phi_s"], g["phi_n"], 0, loading)
        assert v.ok, v.message


# ---- memory contract and refusals ------------------------------------------------------------------------------------
GUARD = 256


class Guarded:
    """A device buffer of `count` elements between two guards, all of it a sentinel."""
    def __init__(self, count, dtype, fill):
        self.t = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.count, self.fill = count, fill
        self.before = self.t.clone()

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())

    def region(self):
        return self.t[GUARD:GUARD + self.count]

    def guards_intact(self):
        return bool(torch.equal(self.t[:GUARD].view(torch.uint8), self.before[:GUARD].view(torch.uint8)) and
                    torch.equal(self.t[GUARD + self.count:].view(torch.uint8), self.before[GUARD + self.count:].view(torch.uint8)))

    def untouched(self):
        return bool(torch.equal(self.t.view(torch.uint8), self.before.view(torch.uint8)))


def contract_case(C=3):
    clips = [M.random_clip(T, C, 7500 + T, tail) for T, tail in ((5, 17), (33, 0), (1, 159))]
    masks = [M.random_mask(len_t, 7600 + len_t) for len_t in (5, 33, 1)]
    off = context.offsets(len(x) for x in clips)
    foff = context.offsets((5, 33, 1))
    planes = torch.from_numpy(np.concatenate([mvdr.planes(x) for x in clips])).cuda()
    mask = torch.from_numpy(np.concatenate(masks)).cuda()
    return clips, masks, off, foff, planes, mask


def outputs(C, n, F):
    f32, f64 = 3.5e13, 1.7e130
    return {"X": Guarded(2 * C * F * BINS, torch.float32, f32), "clm": Guarded(C * F * BINS, torch.float32, f32),
            "cph": Guarded(C * F * BINS, torch.float32, f32), "w": Guarded(2 * n * BINS * C, torch.float64, f64),
            "cov": Guarded(4 * n * C * C * BINS, torch.float64, f64), "rec": Guarded(n * hip.MVDR_FIELDS, torch.float64, f64),
            "lm": Guarded(F * BINS, torch.float32, f32), "ph": Guarded(F * BINS, torch.float32, f32), "y": Guarded(2 * F * BINS, torch.float32, f32)}


def test_outputs_only_are_written_and_inputs_only_read(eng):
    C = 3
    clips, masks, off, foff, planes, mask = contract_case(C)
    n, F = len(clips), foff[-1]
    o = outputs(C, n, F)
    keep = [planes.clone(), mask.clone()]
    lib, h, s = eng.lib, eng.handle, eng._stream()
    so, fo = hip.i64_array(off), hip.i64_array(foff)
    hip.check(lib.nhans_mvdr_spectra(h, hip.ptr(planes), so, n, C, o["X"].ptr(), o["clm"].ptr(), o["cph"].ptr(), s))
    hip.check(lib.nhans_mvdr_weights(h, o["X"].ptr(), hip.ptr(mask), fo, n, C, 1, 1e-6, 0, o["w"].ptr(), o["cov"].ptr(), o["rec"].ptr(), s))
    hip.check(lib.nhans_mvdr_apply(h, o["X"].ptr(), o["w"].ptr(), None, fo, n, C, o["lm"].ptr(), o["ph"].ptr(), o["y"].ptr(), o["rec"].ptr(), s))
    torch.cuda.synchronize()
    for k, g in o.items():
        assert g.guards_intact(), k
        r = g.region()
        assert bool(torch.isfinite(r).all()) and not bool((r == g.fill).any()), "%s: a hole or a sentinel left" % k
    assert torch.equal(planes, keep[0]) and torch.equal(mask, keep[1])
    # the one-call path on fresh guarded outputs: the same bits, the same contract
    p = outputs(C, n, F)
    hip.check(lib.nhans_mvdr(h, hip.ptr(planes), so, n, C, hip.ptr(mask), 1, 1e-6, 0, None, p["lm"].ptr(), p["ph"].ptr(), p["w"].ptr(),
                             p["rec"].ptr(), s))
    torch.cuda.synchronize()
    for k in ("lm", "ph", "w", "rec"):
        assert p[k].guards_intact() and torch.equal(p[k].region().view(torch.uint8), o[k].region().view(torch.uint8)), k
    for k in ("X", "clm", "cph", "cov", "y"):
        assert p[k].untouched(), k
    assert torch.equal(planes, keep[0]) and torch.equal(mask, keep[1])


def test_every_refusal_comes_before_a_launch_and_writes_nothing(eng):
    C = 3
    clips, masks, off, foff, planes, mask = contract_case(C)
    n, F = len(clips), foff[-1]
    o = outputs(C, n, F)
    lib, h, s = eng.lib, eng.handle, eng._stream()
    wd = torch.zeros(2 * n * BINS * C, dtype=torch.float64, device="cuda")
    good = dict(C=C, ref=1, loading=1e-6, flags=0, off=off, foff=foff, planes=hip.ptr(planes), mask=hip.ptr(mask), n=n)
    down = list(off); down[2] = down[1] - 1
    fdown = list(foff); fdown[2] = fdown[1] - 1
    short = list(off); short[1] = off[0] + 399; short[2] = max(short[2], short[1])
    fshort = [0, 5, 5, 6]
    bad = [("C = 0", dict(C=0, ref=0)), ("C = 9", dict(C=9)), ("ref = C", dict(ref=C)), ("ref = -1", dict(ref=-1)), ("loading > 1", dict(loading=1.5)),
           ("loading < 0", dict(loading=-1e-9)), ("loading NaN", dict(loading=float("nan"))), ("flag bits", dict(flags=2)),
           ("null planes", dict(planes=None)), ("null mask", dict(mask=None)), ("descending offsets", dict(off=down, foff=fdown)),
           ("a clip without a frame", dict(off=short, foff=fshort)), ("negative count", dict(n=-1))]
    eng.profile_reset()
    eng.set_option("profile", 1)
    try:
        for name, change in bad:
            a = dict(good, **change)
            so, fo = hip.i64_array(a["off"]), hip.i64_array(a["foff"])
            calls = []
            if not {"mask", "ref", "loading", "flags"} & set(change):
                calls.append(("spectra", lambda: lib.nhans_mvdr_spectra(h, a["planes"], so, a["n"], a["C"], o["X"].ptr(), o["clm"].ptr(), o["cph"].ptr(), s)))
            if "planes" not in change:
                calls.append(("weights", lambda: lib.nhans_mvdr_weights(h, hip.ptr(planes), a["mask"], fo, a["n"], a["C"], a["ref"], a["loading"], a["flags"],
                                                                       o["w"].ptr(), o["cov"].ptr(), o["rec"].ptr(), s)))
            if not {"mask", "ref", "loading", "flags", "planes"} & set(change):
                calls.append(("apply", lambda: lib.nhans_mvdr_apply(h, hip.ptr(planes), hip.ptr(wd), None, fo, a["n"], a["C"], o["lm"].ptr(),
                                                                   o["ph"].ptr(), o["y"].ptr(), o["rec"].ptr(), s)))
            calls.append(("mvdr", lambda: lib.nhans_mvdr(h, a["planes"], so, a["n"], a["C"], a["mask"], a["ref"], a["loading"], a["flags"], None,
                                                         o["lm"].ptr(), o["ph"].ptr(), o["w"].ptr(), o["rec"].ptr(), s)))
            for which, call in calls:
                rc = call()
                msg = lib.nhans_last_error().decode()
                assert rc == -1, (name, which, rc)
                assert "nhans_mvdr" in msg, (name, which, msg)
                if name == "a clip without a frame":
                    assert ("clip 1 has no frame" if which in ("weights", "apply") else "clip 0 has no frame") in msg, msg
        for which, call in (("weights, null w", lambda: lib.nhans_mvdr_weights(h, hip.ptr(planes), hip.ptr(mask), hip.i64_array(foff), n, C, 0, 0.0, 0, None,
                                                                              None, None, s)),
                            ("apply, null rows", lambda: lib.nhans_mvdr_apply(h, hip.ptr(planes), hip.ptr(wd), None, hip.i64_array(foff), n, C,
                                                                              None, o["ph"].ptr(), None, None, s)),
                            ("mvdr, null rows", lambda: lib.nhans_mvdr(h, hip.ptr(planes), hip.i64_array(off), n, C, hip.ptr(mask), 0, 0.0, 0, None, o["lm"].ptr(),
                                                                       None, None, None, s))):
            assert call() == -1, which
        torch.cuda.synchronize()
        prof = eng.profile()
    finally:
        eng.set_option("profile", 0)
    assert "mvdr" not in str(prof), prof             # no launch was recorded
    for k, g in o.items():
        assert g.untouched(), k


# ---- end to end ---------------------------------------------------------------------------------------------------
def demo_inputs():
    sc = M.scene("example2", 2)
    x = (sc["x"] / np.float32(np.abs(sc["x"]).max() + 1e-6)).astype(np.float32)
    return x, O.normalise(synth.silent()), O.normalise(synth.noise_context(1))


@pytest.mark.parametrize("post", ["none", "mask", "net"])
def test_enhance_array_is_the_composition_of_the_public_calls(eng, post):
    """C = 2 on the 1.4 s clip, synthetic weights, the mask from the channels' mean, ref = 1, two Griffin-Lim iterations."""
    x, pos, neg = demo_inputs()
    n, C = x.shape
    got = eng.enhance_array([x], [pos], [neg], ref=1, mask_from="mean", post=post, phase_iters=2, taps=True)
    planes = torch.from_numpy(mvdr.planes(x)).cuda()
    mean = torch.empty(n, dtype=torch.float32, device="cuda")
    hip.check(eng.lib.nhans_channel_mean(eng.handle, hip.ptr(planes), C, n, hip.ptr(mean), eng._stream()))
    assert bits(mean.cpu().numpy()) == bits(x.astype(np.float64).mean(axis=1).astype(np.float32))    # today's signal, bit for bit
    lm, ph = eng.stft_features(mean, [0, n])
    T = lm.shape[0]
    ctx = [eng.stft_features(torch.from_numpy(c).cuda(), [0, len(c)], max_frames=spec.NOISE_WIN, want_phase=False)[0] for c in (pos, neg)]
    emb = eng.embed(torch.stack(ctx))
    logits, _ = eng.mask_net(lm, [0, T], emb[0:1], emb[1:2])
    bf = eng.mvdr_device(planes, [0, n], C, logits, ref=1, loggain=True, gain_t=logits if post == "mask" else None)
    rows = eng.mask_net(bf["logmag"].contiguous(), [0, T], emb[0:1], emb[1:2], want_logits=False)[1] if post == "net" else bf["logmag"].contiguous()
    rph = eng.phase_refine_rows(rows, bf["phase"].contiguous(), [0, T], 2)
    wav, _ = eng.istft(rows, rph, [0, T])
    assert bits(got["logits"][0]) == bits(logits.cpu().numpy())
    assert bits(got["bf_logmag"][0]) == bits(bf["logmag"].cpu().numpy()) and bits(got["bf_phase"][0]) == bits(bf["phase"].cpu().numpy())
    assert bits(got["logmag"][0]) == bits(rows.cpu().numpy()) and bits(got["phase"][0]) == bits(rph.cpu().numpy())
    assert bits(got["denoised_wav"][0]) == bits(wav.cpu().numpy())
    assert got["records"][0] == mvdr.record(bf["records"][0].cpu().numpy())
    assert np.isfinite(got["denoised_wav"][0]).all() and len(got["denoised_wav"][0]) == n
    # the mask from one channel: a different signal through the same calls
    other = eng.enhance_array([x], [pos], [neg], ref=1, mask_from=0, post=post)
    assert np.isfinite(other["denoised_wav"][0]).all() and bits(other["denoised_wav"][0]) != bits(got["denoised_wav"][0])
    print("post=%s: fallback bins %d, energy out / ref %.3f" % (post, got["records"][0]["fallback_bins"],
                                                               got["records"][0]["energy_out"] / got["records"][0]["energy_ref"]))


@pytest.mark.parametrize("name", M.SCENES)
@pytest.mark.parametrize("C", [2, 4])
def test_array_ceiling_on_the_scenes(eng, name, C):
    """The device's four figures per mask within 0.05 dB of float64 (the margin phase_ceiling holds), and the condition of
    tests/test_mvdr_host.py on the device's own figures."""
    sc = M.scene(name, C)
    figs = {}
    for which in ("trained_mask", "oracle_mask"):
        want = M.scene_scores(sc, sc[which])
        got = apply.array_ceiling(eng, sc["x"], sc["target_image"].astype(np.float32), sc[which], edge=M.EDGE)
        figs[which] = got
        print("%s C %d %-12s device: channel 0 %.2f, mean %.2f, mask alone %.2f, MVDR %.2f dB; float64: %.2f, %.2f, %.2f, %.2f; fallback %d" % (
            name, C, which, got["ref"]["si_sdr_db"], got["mean"]["si_sdr_db"], got["mask"]["si_sdr_db"], got["mvdr"]["si_sdr_db"],
            want["ref"], want["mean"], want["mask"], want["mvdr"], got["fallback_bins"]))
        for k in ("ref", "mean", "mask", "mvdr"):
            assert abs(got[k]["si_sdr_db"] - want[k]) <= 0.05, (which, k)
        assert got["fallback_bins"] == want["fallback_bins"] == 0
    tr, orc = figs["trained_mask"], figs["oracle_mask"]
    assert tr["mvdr"]["si_sdr_db"] - max(tr["ref"]["si_sdr_db"], tr["mean"]["si_sdr_db"]) >= M.MARGIN_DB
    assert orc["mvdr"]["si_sdr_db"] - tr["mask"]["si_sdr_db"] >= M.MARGIN_DB


# ---- the command line ------------------------------------------------------------------------------------------------
def test_cli_array_flag_beamforms_and_its_absence_changes_nothing(eng, tmp_path, capsys):
    """File and directory mode on stereo files: with --array mvdr the files are enhance_array's of the channels the reader
    keeps; without it they are byte for byte what enhance gives for the channels' mean, as always."""
    from scipy.io import wavfile
    eng.set_precision("f16x3")
    apply.set_engine("denoiser", eng)
    keep = dict(vars(apply.FLAGS))
    try:
        sc = M.scene("example2", 2)
        pcm = np.clip(np.round(sc["x"] / np.abs(sc["x"]).max() * 20000.0), -32768, 32767).astype(np.int16)
        noise = synth.noise_context(41, 1.0)
        ind, negd = tmp_path / "in", tmp_path / "neg"
        ind.mkdir(), negd.mkdir()
        for name, k in (("a.wav", len(pcm)), ("b.wav", len(pcm) - 1000)):
            wavfile.write(str(ind / name), 16000, pcm[:k])
            wavfile.write(str(negd / name), 16000, noise)
        common = ["--pos", str(tmp_path / "Silent.wav"), "--weights", "synthetic"]
        one = ["--input", str(ind / "a.wav"), "--neg", str(negd / "a.wav")]
        apply.main(one + ["--output", str(tmp_path / "plain.wav")] + common)
        apply.main(one + ["--output", str(tmp_path / "bf.wav"), "--array", "mvdr", "--array_ref", "1", "--array_post", "mask"] + common)
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "dplain")] + common)
        apply.main(["--input", str(ind), "--neg", str(negd), "--output", str(tmp_path / "dbf"), "--array", "mvdr", "--array_ref", "1",
                    "--array_post", "mask"] + common)
        capsys.readouterr()
        for k, v in keep.items():
            setattr(apply.FLAGS, k, v)
        # without the flag: the channels' mean through enhance, as before
        pos, neg, mixed = apply.handle_signals(str(ind / "a.wav"), None, str(negd / "a.wav"))
        want = eng.enhance([mixed], [pos], [neg], want_mixed=True)
        rate, got = wavfile.read(str(tmp_path / "plain.wav"))
        assert rate == 16000 and bits(got) == bits(want["denoised_wav"][0])
        assert bits(wavfile.read(str(tmp_path / "plain_mixed_processed.wav"))[1]) == bits(want["mixed_wav"][0])
        # with it: enhance_array of the kept channels
        ca, cb, x = apply.handle_array_signals(str(ind / "a.wav"), None, str(negd / "a.wav"))
        assert x.shape == (len(mixed), 2)
        bf = eng.enhance_array([x], [ca], [cb], ref=1, post="mask", want_mixed=True)
        got_bf = wavfile.read(str(tmp_path / "bf.wav"))[1]
        assert bits(got_bf) == bits(bf["denoised_wav"][0]) and bits(got_bf) != bits(got)
        assert bits(wavfile.read(str(tmp_path / "bf_mixed_processed.wav"))[1]) == bits(bf["mixed_wav"][0])
        # directory mode: the same files as file mode, both ways
        for d, f in (("dplain", "plain"), ("dbf", "bf")):
            for tail in (".wav", "_mixed_processed.wav", "_removed.wav", "_compensated.wav"):
                assert open(str(tmp_path / d / ("a" + tail)), "rb").read() == open(str(tmp_path / (f + tail)), "rb").read(), (d, tail)
            assert (tmp_path / d / "b.wav").exists()
        # a mono input with the flag is an argument error
        wavfile.write(str(tmp_path / "mono.wav"), 16000, pcm[:, 0].copy())
        with pytest.raises(SystemExit) as e:
            apply.main(["--input", str(tmp_path / "mono.wav"), "--output", str(tmp_path / "m.wav"), "--array", "mvdr"] + common)
        assert e.value.code == 2 and "is mono" in capsys.readouterr().err
        assert not (tmp_path / "m.wav").exists()
    finally:
        apply._engines.pop("denoiser", None)
        for k, v in keep.items():
            setattr(apply.FLAGS, k, v)
