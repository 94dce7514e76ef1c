"""Every entry point of include/nhans_hip.h that takes caller-owned device buffers writes its outputs only and reads its
inputs only (tests/memory_checks.py has the rule and the helper).  One test per entry point, each with the same three
assertions over three runs of the same call through the C ABI, so that the test owns every pointer:

    "exact"  exact-size outputs, tightly packed offsets, inputs with zero surroundings, everything 16-byte aligned -- the
             buffers the Python wrappers make, whose bits the parity tests of the suite already hold to their references;
    "A"      outputs in guarded buffers (sentinel 0) with rooms larger than the counts and odd gaps between clips, inputs
             surrounded by zeros, both off the 16-byte boundary;
    "B"      the same with sentinel 1 and inputs surrounded by poison.

 (a) no finding from the guarded outputs of A and B: no guard word and no slack element changed, and no documented element
     holds the sentinel in both;  (b) the documented ranges of A hold the bits of "exact";  (c) those of B hold the bits of A.
Every buffer is larger than what the library is told: a stray store or load stays inside memory the test owns.
"""
import ctypes

import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import hip, resample, score, spec

import memory_checks as MC

pytestmark = pytest.mark.gpu

LAYOUTS = ("exact", "A", "B")


@pytest.fixture(scope="module")
def eng(lib_built, weights_denoiser):
    from nhans_amd import engine
    e = engine.Engine("denoiser", weights_denoiser, precision="f16x3")
    yield e
    e.close()


_hip_error = []


@pytest.fixture(autouse=True)
def _nothing_after_a_hip_error():
    """A HIP error (a launch refused, a fault at a synchronisation) ends this module: later tests start nothing on the device."""
    if _hip_error:
        pytest.fail("an earlier test of this module met a HIP error (%s): not run" % _hip_error[0])
    yield


def _sync():
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _hip_error.append(str(e).splitlines()[0])
        raise


def _ok(rc, what=""):
    if rc == -2:
        _hip_error.append("%s: %s" % (what, hip.load().nhans_last_error()))
    assert rc == 0, "%s: %s" % (what, hip.load().nhans_last_error())
    return True


# ---- the three-run driver -------------------------------------------------------------------------------------------------
class In:
    """An input of contiguous clips (clip c owns [off[c], off[c + 1]) of the buffer).  dead: clips the call names in its
    offsets and never reads -- a gap between live clips, poisoned in variant B.  unit: elements per offset unit (the channels of
    an interleaved frame)."""

    def __init__(self, kind, pieces, poison=None, dead=(), unit=1):
        self.kind, self.poison, self.dead, self.unit = kind, poison, set(dead), unit
        self.pieces = [np.ascontiguousarray(p, dtype=MC.KINDS[kind][0]).reshape(-1) for p in pieces]
        self.offsets = MC.tight_offsets([len(p) for p in self.pieces])

    def build(self, layout, align, device):
        live = [c for c in range(len(self.pieces)) if c not in self.dead]
        buf = MC.Surrounded(self.kind, [self.pieces[c] for c in live], [self.offsets[c] for c in live], size=self.offsets[-1],
                            align=align % MC.lanes(self.kind) if layout != "exact" else 0,
                            variant="B" if layout == "B" else "A", poison=self.poison, device=device)
        assert all(o % self.unit == 0 for o in self.offsets)
        return Built(buf, [o // self.unit for o in self.offsets], None, self.offsets)


class Out:
    """An output.  counts: ragged -- clip c writes counts[c] elements at its offset (tight offsets in "exact", rooms with odd
    slack otherwise).  size + mask: a fixed layout the call derives itself (records, rows packed clip after clip); the guarded
    runs add `tail` slack elements behind it."""

    def __init__(self, kind, counts=None, size=None, mask=None, tail=3, unit=1):
        self.kind, self.counts, self.tail, self.unit = kind, counts, tail, unit
        if counts is None:
            self.mask = np.ones(int(size), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
            assert len(self.mask) == int(size)

    def build(self, layout, align, device):
        guarded = layout != "exact"
        if self.counts is not None:
            off = MC.ragged_offsets(self.counts, self.kind) if guarded else MC.tight_offsets(self.counts)
            eoff = [o * self.unit for o in off]
            mask = MC.prefix_mask(eoff, [n * self.unit for n in self.counts])
        else:
            off = eoff = None
            mask = np.concatenate([self.mask, np.zeros(self.tail if guarded else 0, dtype=bool)])
        buf = MC.Guarded(self.kind, len(mask), align=align % MC.lanes(self.kind) if guarded else 0, which=int(layout == "B"),
                         device=device)
        return Built(buf, off, mask, eoff)


class Built:
    def __init__(self, buf, offsets, mask, eoffsets):
        self.buf, self.offsets, self.mask, self.eoffsets = buf, offsets, mask, eoffsets     # offsets: in the call's units


class Bufs:
    def __init__(self, layout, built):
        self.layout, self.built = layout, built

    def p(self, name, element=0):
        b = self.built.get(name)
        return None if b is None else ctypes.c_void_p(b.buf.element_ptr(element))

    def o(self, name):
        return hip.i64_array(self.built[name].offsets)

    def offsets(self, name):
        return self.built[name].offsets


class Contract:
    def __init__(self, eng, in_align=1, out_align=1):
        self.eng, self.in_align, self.out_align = eng, in_align, out_align
        self.runs = {k: [] for k in LAYOUTS}

    def buffers(self, layout, ins, outs):
        """ins / outs: name -> In / Out (None: a NULL pointer).  Successive buffers of a call get successive alignments."""
        built = {}
        for j, (k, s) in enumerate(ins.items()):
            built[k] = s.build(layout, self.in_align + j, self.eng.device) if s is not None else None
        for j, (k, s) in enumerate(outs.items()):
            built[k] = s.build(layout, self.out_align + j, self.eng.device) if s is not None else None
        b = Bufs(layout, built)
        self.runs[layout].append((b, [k for k, s in outs.items() if s is not None]))
        return b

    def check(self, what=""):
        _sync()
        n = len(self.runs["exact"])
        assert n and all(len(self.runs[k]) == n for k in LAYOUTS)
        for i in range(n):
            (e, names), (a, _), (b, _) = (self.runs[k][i] for k in LAYOUTS)
            for name in names:
                E, A, B = e.built[name], a.built[name], b.built[name]
                where = "%s call %d output %s" % (what, i, name)
                f = MC.findings([A.buf, B.buf], A.mask, A.eoffsets)
                assert not f, "%s: %s" % (where, MC.report(f))                                              # (a)
                assert E.mask.sum() == A.mask.sum()
                de, da, db = E.buf.region_bits()[E.mask], A.buf.region_bits()[A.mask], B.buf.region_bits()[B.mask]
                assert np.array_equal(da, de), "%s: %d documented elements differ from the exact-size call, first %d" % (
                    where, int((da != de).sum()), int(np.flatnonzero(da != de)[0]))                         # (b)
                assert np.array_equal(db, da), "%s: %d documented elements follow the inputs' surroundings, first %d" % (
                    where, int((db != da).sum()), int(np.flatnonzero(db != da)[0]))                         # (c)
        return self.runs


def run_contract(eng, ins, outs, call, what="", in_align=1, out_align=1):
    """call(bufs) -> the library's return code.  One call per layout, then the three assertions."""
    c = Contract(eng, in_align, out_align)
    for layout in LAYOUTS:
        b = c.buffers(layout, ins, outs)
        _ok(call(b), "%s (%s)" % (what, layout))
    return c.check(what)


def _rng(seed):
    return np.random.default_rng(seed)


def _pcm(rng, n, kind):
    if kind == "i16":
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return (rng.standard_normal(n) * 8000.0).astype(np.float32)


FORMAT = {"i16": hip.PCM_INT16, "f32": hip.PCM_FLOAT32}


# ---- sample-rate conversion ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("pair", [(48000, 16000), (16000, 44100), (16000, 16000)], ids=lambda p: "%d-%d" % p)
def test_resample(eng, pair, kind):
    lib = hip.load()
    J = resample.geometry(*pair)[3] if pair[0] != pair[1] else 2
    lens = [0, 1, max(J - 1, 1), 257, 1025]
    rng = _rng(11)
    clips = [_pcm(rng, n, kind) for n in lens]
    counts = [resample.out_count(n, *pair) for n in lens]
    for k, flags in enumerate((0, hip.RESAMPLE_QUANTISE)):
        run_contract(eng, {"in": In(kind, clips)}, {"out": Out("f32", counts)},
                     lambda b: lib.nhans_resample(eng.handle, b.p("in"), FORMAT[kind], b.o("in"), len(lens), pair[0], pair[1], flags,
                                                  b.p("out"), b.o("out"), eng._stream()),
                     "nhans_resample flags %d" % flags, in_align=1 + 2 * k, out_align=3 - k)


def test_stoi_resample(eng):
    lib = hip.load()
    lens = [0, 1, 7, 1030]
    rng = _rng(12)
    clips = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    counts = [int(lib.nhans_stoi_out_count(n)) for n in lens]
    for align in (1, 3):
        run_contract(eng, {"in": In("f32", clips)}, {"out": Out("f32", counts)},
                     lambda b: lib.nhans_stoi_resample(eng.handle, b.p("in"), b.o("in"), len(lens), b.p("out"), b.o("out"), eng._stream()),
                     "nhans_stoi_resample", in_align=align, out_align=4 - align)


def test_resample_checker_sees_one_element_on_the_device(eng):
    """The sensitivity check: no kernel is touched, the checker is told a count one less / one more than the true one for
    the middle clip and must report exactly one slack element written / exactly one hole, at that clip."""
    lib = hip.load()
    lens = [300, 257, 129]
    rng = _rng(13)
    clips = In("i16", [_pcm(rng, n, "i16") for n in lens])
    counts = [resample.out_count(n, 48000, 16000) for n in lens]
    off = MC.ragged_offsets(counts, "f32")
    src = clips.build("A", 1, eng.device)
    runs = []
    for which in (0, 1):
        g = MC.Guarded("f32", off[-1], align=3, which=which, device=eng.device)
        assert lib.nhans_resample(eng.handle, ctypes.c_void_p(src.buf.ptr), hip.PCM_INT16, hip.i64_array(src.offsets), 3, 48000, 16000, 0,
                                  ctypes.c_void_p(g.ptr), hip.i64_array(off), eng._stream()) == 0
        runs.append(g)
    _sync()
    assert MC.findings(runs, MC.prefix_mask(off, counts), off) == []
    less = MC.findings(runs[0], MC.prefix_mask(off, [counts[0], counts[1] - 1, counts[2]]), off)
    assert len(less) == 1 and less[0][:4] == ("slack", 1, off[1] + counts[1] - 1, 1), less
    more = MC.findings(runs, MC.prefix_mask(off, [counts[0], counts[1] + 1, counts[2]]), off)
    assert len(more) == 1 and more[0][:4] == ("hole", 1, off[1] + counts[1], 1), more
    # assertion (c) sees a load one element outside a range: the last clip is DECLARED one sample longer -- a sample the test
    # owns, 0 in variant A and full scale in variant B -- and the two variants' outputs differ
    assert resample.out_count(lens[2] + 1, 48000, 16000) <= off[3] - off[2]
    outs, srcs = [], []
    longer = src.offsets[:3] + [src.offsets[3] + 1]
    for layout in ("A", "B"):
        srcs.append(clips.build(layout, 1, eng.device))
        g = MC.Guarded("f32", off[-1], align=3, device=eng.device)
        assert lib.nhans_resample(eng.handle, ctypes.c_void_p(srcs[-1].buf.ptr), hip.PCM_INT16, hip.i64_array(longer), 3, 48000, 16000, 0,
                                  ctypes.c_void_p(g.ptr), hip.i64_array(off), eng._stream()) == 0
        outs.append(g)
    _sync()
    assert np.array_equal(outs[0].region_bits()[:off[2]], outs[1].region_bits()[:off[2]])
    assert not np.array_equal(outs[0].region_bits()[off[2]:], outs[1].region_bits()[off[2]:])


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_resampler_push(eng, kind):
    """3 streams 48000 -> 16000, pushes of 0, 1, 7 and 480 samples in turn, stream 1 ends early; every push is a call of its own
    with its own guarded output and its own surrounded input pieces."""
    lib = hip.load()
    S, pair = 3, (48000, 16000)
    rng = _rng(14)
    sizes = [[0, 1, 7], [480, 480, 480], [1, 7, 0], [7, 0, 480], [480, 0, 1], [480, 0, 480]]
    ends = [None, None, None, [0, 1, 0], None, [1, 0, 1]]
    data = [[_pcm(rng, n, kind) for n in row] for row in sizes]
    c = Contract(eng)
    for layout in LAYOUTS:
        h = ctypes.c_void_p()
        assert lib.nhans_resampler_open(eng.handle, S, pair[0], pair[1], FORMAT[kind], 0, ctypes.byref(h)) == 0
        try:
            for row, end in zip(data, ends):
                endv = (ctypes.c_int * S)(*end) if end else None
                want = (ctypes.c_int64 * S)()
                assert lib.nhans_resampler_out_counts(h, hip.i64_array([len(p) for p in row]), endv, want) == 0
                b = c.buffers(layout, {"in": In(kind, row)}, {"out": Out("f32", list(want))})
                got = (ctypes.c_int64 * S)()
                _ok(lib.nhans_resampler_push(h, b.p("in"), b.o("in"), endv, b.p("out"), b.o("out"), got, eng._stream()))
                assert list(got) == list(want)
            _sync()
        finally:
            lib.nhans_resampler_close(h)
    c.check("nhans_resampler_push %s" % kind)


@pytest.mark.parametrize("flags", [0, hip.NORMALISE_WRAP_INT16])
def test_peak_normalise(eng, flags):
    """Input and output share one offset array, so the rooms are exact: the guards and a tail of slack are what is watched."""
    lib = hip.load()
    lens = [0, 1, 255, 256, 257, 8193]
    rng = _rng(15)
    clips = [_pcm(rng, n, "f32").round() for n in lens]
    clips[3][5] = -32768.0                                  # the peak the wrap flag reads as negative
    total = sum(lens)
    for align in (1, 2):
        src = In("f32", clips)
        run_contract(eng, {"in": src}, {"out": Out("f32", size=total)},
                     lambda b: lib.nhans_peak_normalise(eng.handle, b.p("in"), b.o("in"), len(lens), flags, b.p("out"), eng._stream()),
                     "nhans_peak_normalise", in_align=align, out_align=align + 1)
    # in place inside one guarded buffer: the exact call's bits, guards and tail intact under both sentinels
    ref = run_contract(eng, {"in": In("f32", clips)}, {"out": Out("f32", size=total)},
                       lambda b: lib.nhans_peak_normalise(eng.handle, b.p("in"), b.o("in"), len(lens), flags, b.p("out"), eng._stream()),
                       "nhans_peak_normalise")["exact"][0][0].built["out"].buf.region_bits()
    mask = np.concatenate([np.ones(total, dtype=bool), np.zeros(5, dtype=bool)])
    runs = []
    for which in (0, 1):
        g = MC.Guarded("f32", total + 5, align=3, which=which, device=eng.device)
        g.place(0, np.concatenate(clips))
        assert lib.nhans_peak_normalise(eng.handle, ctypes.c_void_p(g.ptr), hip.i64_array(MC.tight_offsets(lens)), len(lens), flags,
                                        ctypes.c_void_p(g.ptr), eng._stream()) == 0
        runs.append(g)
    _sync()
    f = MC.findings(runs, mask)
    assert not f, MC.report(f)
    for g in runs:
        assert np.array_equal(g.region_bits()[:total], ref)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_channel_mean(eng, C):
    lib = hip.load()
    rng = _rng(16)
    for k, n in enumerate((1, 255, 256, 257)):
        planes = [_pcm(rng, n, "f32") for _ in range(C)]
        res = run_contract(eng, {"in": In("f32", planes)}, {"out": Out("f32", size=n)},
                           lambda b: lib.nhans_channel_mean(eng.handle, b.p("in"), C, n, b.p("out"), eng._stream()),
                           "nhans_channel_mean C %d n %d" % (C, n), in_align=k, out_align=k + 1)
        ref = res["exact"][0][0].built["out"].buf.region_bits()
        # in place: plane 0 becomes the mean, planes 1 .. C - 1 and everything around keep their bits
        runs = []
        for which in (0, 1):
            g = MC.Guarded("f32", C * n + 3, align=(k + 2) % 4, which=which, device=eng.device)
            g.place(0, np.concatenate(planes))
            assert lib.nhans_channel_mean(eng.handle, ctypes.c_void_p(g.ptr), C, n, ctypes.c_void_p(g.ptr), eng._stream()) == 0
            runs.append(g)
        _sync()
        f = MC.findings(runs, np.concatenate([np.ones(C * n, dtype=bool), np.zeros(3, dtype=bool)]))
        assert not f, MC.report(f)
        for g in runs:
            assert np.array_equal(g.region_bits()[:n], ref)
            assert MC.same_bits(g.region()[n:C * n], np.concatenate(planes)[n:])


# ---- level meter ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [0, 4])
def test_level_gains(eng, W):
    lib = hip.load()
    lens = [0, 1, 160, 161, 256 * 160 + 5]
    rng = _rng(17)
    den = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    mix = [(d + 0.05 * rng.standard_normal(len(d))).astype(np.float32) for d in den]
    hops = [-(-n // 160) for n in lens]
    sums = np.ones((len(lens), 8), dtype=bool)
    sums[0] = False                                          # nothing for an empty clip
    for align in (1, 2):
        run_contract(eng, {"den": In("f32", den), "mix": In("f32", mix)},
                     {"w": Out("f32", size=sum(hops)), "sums": Out("f64", size=sums.size, mask=sums)},
                     lambda b: lib.nhans_level_gains(eng.handle, b.p("den"), b.p("mix"), b.o("den"), len(lens), W, 1.0, b.p("w"),
                                                     b.p("sums"), eng._stream()),
                     "nhans_level_gains W %d" % W, in_align=align, out_align=align)


# ---- filterbank ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bank", ["htk80", "custom"])
def test_fbank_rows(eng, bank):
    import fbank_checks as FC
    lib = hip.load()
    fb = FC.bank(bank)
    h = fb.handle(eng)
    for nrows in (1, 15, 16, 17, 33):
        rows = FC.uniform_rows(nrows, seed=nrows)
        for align in (0, 1):
            run_contract(eng, {"rows": In("f32", [rows], poison="big")}, {"out": Out("f32", size=nrows * fb.n_mels)},
                         lambda b: lib.nhans_fbank_rows(h, b.p("rows"), nrows, b.p("out"), eng._stream()),
                         "nhans_fbank_rows %s rows %d" % (bank, nrows), in_align=align, out_align=align + nrows)


# ---- scoring -------------------------------------------------------------------------------------------------------------
def test_score_wave(eng):
    lib = hip.load()
    T = hip.SCORE_TILE
    lens = [1, 399, 400, T - 1, T + 1, 0, 3 * 160 + 400]
    rng = _rng(18)
    tgt = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    est = [(t + 0.05 * rng.standard_normal(len(t))).astype(np.float32) for t in tgt]
    est[4] = np.concatenate([est[4], np.ones(9, np.float32)])        # a longer estimate: the common prefix counts
    tgt[6] = np.concatenate([tgt[6], np.ones(170, np.float32)])      # a longer target
    frames = [int(lib.nhans_num_frames(n)) for n in lens]
    fmask = np.zeros((sum(frames), 3), dtype=bool)
    fmask[:, 0] = True                                               # columns 1 - 2 are nhans_score_rows'
    for align in (1, 3):
        run_contract(eng, {"est": In("f32", est), "tgt": In("f32", tgt)},
                     {"rec": Out("f64", size=len(lens) * hip.SCORE_FIELDS), "frames": Out("f64", size=fmask.size, mask=fmask)},
                     lambda b: lib.nhans_score_wave(eng.handle, b.p("est"), b.o("est"), b.p("tgt"), b.o("tgt"), len(lens), b.p("rec"),
                                                    b.p("frames"), eng._stream()),
                     "nhans_score_wave", in_align=align, out_align=1)


def test_score_rows(eng):
    lib = hip.load()
    nrows = [0, 1, 15, 16, 17]
    rng = _rng(19)
    tgt = [rng.uniform(-12.0, 3.0, size=(n, spec.BINS)).astype(np.float32) for n in nrows]
    est = [(t + 0.1 * rng.standard_normal(t.shape)).astype(np.float32) for t in tgt]
    foff = MC.tight_offsets(nrows)
    fmask = np.zeros((sum(nrows), 3), dtype=bool)
    fmask[:, 1:] = True                                              # column 0 is nhans_score_wave's
    for align in (0, 1):
        # (different poisons: with the same one both sides the differences E - T would be zero)
        run_contract(eng, {"est": In("f32", est, poison="big"), "tgt": In("f32", tgt, poison="nan")},
                     {"rec": Out("f64", size=len(nrows) * hip.SCORE_ROW_FIELDS), "frames": Out("f64", size=fmask.size, mask=fmask)},
                     lambda b: lib.nhans_score_rows(eng.handle, b.p("est"), b.p("tgt"), hip.i64_array(foff), len(nrows), b.p("rec"),
                                                    b.p("frames"), eng._stream()),
                     "nhans_score_rows", in_align=align, out_align=1)


# ---- mixing --------------------------------------------------------------------------------------------------------------
def test_mix(eng):
    lib = hip.load()
    T = hip.MIX_TILE
    ns = [1, 2, 3, 5, T - 1, T, T + 1, 2 * T + 3]
    rng = _rng(20)
    speech = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in ns]
    speech.insert(4, np.ones(6, np.float32))                 # speech clip 4 is named by no job: a gap between live clips
    sidx = [0, 1, 2, 3, 5, 6, 7, 8]
    # noises: m = 1 (wrap), n - 1 (wrap), equal, longer; one clip no job names
    nlens = [1, 2, T, T + 1, 7, 2 * T + 2, 2 * T + 3, 3 * T]
    noise = [(0.2 * rng.standard_normal(m)).astype(np.float32) for m in nlens]
    dead_noise = 4
    # (speech, keep, drop, snr_keep, snr_drop)
    jobs = [(0, 0, 1, 0.0, 3.0), (1, 0, 1, -3.0, 0.0), (2, 1, 0, 5.0, 5.0), (3, -1, 0, 0.0, 2.0), (5, 0, 2, 0.0, 0.0),
            (6, 2, 3, 1.0, -1.0), (7, 2, 3, 0.0, 0.0), (8, 5, 7, 2.0, 4.0), (8, 6, 0, 0.0, 6.0), (7, -1, 3, 0.0, 0.0)]
    assert {j[0] for j in jobs} == set(sidx) and dead_noise not in {j[1] for j in jobs} | {j[2] for j in jobs}
    nj = len(jobs)
    si, ki, di = [(ctypes.c_int * nj)(*[j[k] for j in jobs]) for k in range(3)]
    sk, sd = [(ctypes.c_double * nj)(*[j[k] for j in jobs]) for k in (3, 4)]
    counts = [len(speech[j[0]]) for j in jobs]

    def call(b):
        # (the four outputs share ONE offset array: built from the same counts they have the same region-relative offsets, each
        # in a buffer of its own alignment)
        return lib.nhans_mix(eng.handle, b.p("speech"), b.o("speech"), len(speech), b.p("noise"), b.o("noise"), len(noise), si, ki,
                             di, sk, sd, nj, b.p("mixture"), b.p("target"), b.p("keep"), b.p("drop"), b.o("mixture"),
                             b.p("rec"), eng._stream())

    ins = {"speech": In("f32", speech, dead=[4]), "noise": In("f32", noise, dead=[dead_noise])}
    full = None
    for align in range(4):
        outs = {k: Out("f32", counts) for k in ("mixture", "target", "keep", "drop")}
        outs["rec"] = Out("f64", size=nj * hip.MIX_FIELDS)
        res = run_contract(eng, ins, outs, call, "nhans_mix align %d" % align, in_align=align, out_align=align)
        full = full or res
    # the keep output of the two-way jobs is zeros, and written (check() found no hole)
    a = full["A"][0][0].built["keep"]
    for j in (3, 9):
        assert not a.buf.region()[a.offsets[j]:a.offsets[j] + counts[j]].any()
    # target / keep / drop / records NULL: the mixture keeps its bits
    res = run_contract(eng, ins, {"mixture": Out("f32", counts), "target": None, "keep": None, "drop": None, "rec": None}, call,
                       "nhans_mix, optional outputs NULL")
    assert np.array_equal(res["exact"][0][0].built["mixture"].buf.region_bits(), full["exact"][0][0].built["mixture"].buf.region_bits())


# ---- STOI ----------------------------------------------------------------------------------------------------------------
def test_stoi(eng):
    import stoi_checks as SC
    lib = hip.load()
    lens = [0, 256, 385, 4226]
    pairs = [SC.clip(n, 40 + i) for i, n in enumerate(lens)] + [SC.compaction_clip("run_leaves_31")]
    est, tgt = [p[0] for p in pairs], [p[1] for p in pairs]
    assert len(tgt[-1]) == 8000
    est[3] = np.concatenate([est[3], np.ones(11, np.float32)])       # the common prefix counts
    n = [min(len(e), len(t)) for e, t in zip(est, tgt)]
    reserved = [max(score.stoi_num_frames(k) - score.STOI_SEGMENT, 0) for k in n]
    assert reserved == [0, 0, 0, 2, 31]
    refs = [score.stoi_reference(e, t) for e, t in zip(est, tgt)]
    segs = [int(r["segments"]) for r in refs]
    assert segs[3] == 2 and 0 < segs[4] < reserved[4]                # silent frames: rows reserved and not written
    smask = np.zeros((sum(reserved), 2), dtype=bool)
    row = 0
    for r, s in zip(reserved, segs):
        smask[row:row + s] = True
        row += r
    for align in (1, 2):
        run_contract(eng, {"est": In("f32", est), "tgt": In("f32", tgt)},
                     {"rec": Out("f64", size=len(n) * hip.STOI_FIELDS), "seg": Out("f64", size=smask.size, mask=smask)},
                     lambda b: lib.nhans_stoi(eng.handle, b.p("est"), b.o("est"), b.p("tgt"), b.o("tgt"), len(n), b.p("rec"), b.p("seg"),
                                              eng._stream()),
                     "nhans_stoi", in_align=align, out_align=1)


# ---- the tower -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
def test_embed(eng, n):
    import head_checks as H
    lib = hip.load()
    ctx = H.pool_contexts(n).numpy()
    run_contract(eng, {"ctx": In("f32", [ctx], poison="big")}, {"emb": Out("f32", size=n * spec.EMB)},
                 lambda b: lib.nhans_embed(eng.handle, b.p("ctx"), n, b.p("emb"), eng._stream()), "nhans_embed n %d" % n)


# ---- online, live and interleaved sessions --------------------------------------------------------------------------------
def _embeddings(eng, seed=31):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2, spec.EMB, generator=g) * 0.1).to(eng.device).contiguous()


def _ends(S, which):
    return (ctypes.c_int * S)(*[int(s in which) for s in range(S)]) if which else None


PUSHES = 9          # per session; look-aheads of 0 and 2 frames, so that the first final frames come with pushes 4 .. 7


class _Session:
    """One object of `S` slots per layout, conditioned on fixed embeddings, look-ahead (0, 2, 0, 2 ...); pushes in the library's
    own units (samples, or frames of `cin` / `cout` channels)."""

    def __init__(self, eng, contract, layout, opener, names, S, in_kind, out_kinds, cin=1, cout=1):
        self.eng, self.c, self.layout, self.lib, self.names, self.S = eng, contract, layout, hip.load(), names, S
        self.in_kind, self.out_kinds, self.cin, self.cout = in_kind, out_kinds, cin, cout
        self.h = ctypes.c_void_p()
        _ok(opener(ctypes.byref(self.h)), "open")
        self.emb = _embeddings(eng)

    def condition(self, slots, per=1):
        """per: slots per stream (the channels of a split stream share their look-ahead)"""
        L = self.lib
        for s in range(slots):
            _ok(getattr(L, self.names["lookahead"])(self.h, s, (0, 2)[(s // per) % 2]), "look-ahead")
            _ok(getattr(L, self.names["set_embeddings"])(self.h, s, hip.ptr(self.emb[0]), hip.ptr(self.emb[1]), self.eng._stream(), None),
                "set_embeddings")

    def push(self, row, ending=()):
        """row: one array of in-units * cin elements per stream.  -> the counts reported"""
        L, S = self.lib, self.S
        endv = _ends(S, ending)
        want = (ctypes.c_int64 * S)()
        _ok(getattr(L, self.names["out_counts"])(self.h, hip.i64_array([len(p) // self.cin for p in row]), endv, want), "out_counts")
        outs = {k: Out(kind, list(want), unit=self.cout) for k, kind in self.out_kinds.items()}
        b = self.c.buffers(self.layout, {"in": In(self.in_kind, row, unit=self.cin)}, outs)
        got = (ctypes.c_int64 * S)()
        first = next(iter(outs))
        args = [b.p(k) for k in outs] + [b.o(first), got, self.eng._stream()]
        _ok(getattr(L, self.names["push"])(self.h, b.p("in"), b.o("in"), endv, *args), self.names["push"])
        assert list(got) == list(want)
        return list(got)

    def close(self):
        _sync()
        getattr(self.lib, self.names["close"])(self.h)


ONLINE = dict(lookahead="nhans_online_set_lookahead", set_embeddings="nhans_online_set_embeddings", out_counts="nhans_online_out_counts",
              push="nhans_online_push", close="nhans_online_close", fbank_attach="nhans_fbank_online_attach",
              fbank_read="nhans_fbank_online_read", embeddings="nhans_capture_embeddings")
LIVE = dict(lookahead="nhans_lookahead_live_set", set_embeddings="nhans_live_set_embeddings", out_counts="nhans_live_out_counts",
            push="nhans_live_push", close="nhans_live_close", fbank_attach="nhans_fbank_live_attach", fbank_read="nhans_fbank_live_read",
            embeddings="nhans_capture_live_embeddings")
INTERLEAVED = dict(LIVE, out_counts="nhans_interleaved_live_out_counts", push="nhans_interleaved_live_push")


def _online_run(eng, what, after_open=None, after_push=None):
    """2 slots, 160-sample pushes; slot 1 ends with push 7 and takes nothing afterwards, slot 0 ends with the last push."""
    lib = hip.load()
    rng = _rng(21)
    x = [(0.3 * rng.standard_normal(PUSHES * 160)).astype(np.float32) for _ in range(2)]
    c = Contract(eng)
    emitted = None
    for layout in LAYOUTS:
        s = _Session(eng, c, layout, lambda h: lib.nhans_online_open_slots(eng.handle, 2, 1, eng._stream(), h), ONLINE, 2, "f32",
                     {"den": "f32", "mixed": "f32"})
        try:
            s.condition(2)
            if after_open:
                after_open(s)
            counts = []
            for k in range(PUSHES):
                row = [x[0][160 * k:160 * k + 160], x[1][160 * k:160 * k + 160] if k < 7 else x[1][:0]]
                counts.append(s.push(row, ending=[1] if k == 6 else ([0] if k == PUSHES - 1 else [])))
                if after_push:
                    after_push(s)
        finally:
            s.close()
        assert emitted in (None, counts)
        emitted = counts
    # the span crosses the first final frames of both slots and both ends
    first = [min(k for k in range(PUSHES) if emitted[k][i]) for i in (0, 1)]
    assert 0 < first[0] < first[1] < 6 and emitted[6][1] > 320 and emitted[-1][0] > 320, emitted
    c.check(what)


def test_online_push(eng):
    _online_run(eng, "nhans_online_push")


def _read_rows(s, n_mels, slots, planes=(0, 1)):
    """nhans_fbank_*_read of every slot and plane into guarded buffers with room for two rows more than there are."""
    fn = getattr(s.lib, s.names["fbank_read"])
    for slot in range(slots):
        for plane in planes:
            n = fn(s.h, slot, plane, None, 0, None, s.eng._stream())
            assert n >= 0, s.lib.nhans_last_error()
            b = s.c.buffers(s.layout, {}, {"rows": Out("f32", size=n * n_mels, tail=2 * n_mels + 1)})
            first = ctypes.c_int64(-1)
            assert fn(s.h, slot, plane, b.p("rows"), n + 2, ctypes.byref(first), s.eng._stream()) == n and first.value >= 0


def test_fbank_online_read(eng):
    import fbank_checks as FC
    fb = FC.bank("custom")
    _online_run(eng, "nhans_fbank_online_read",
                after_open=lambda s: _ok(s.lib.nhans_fbank_online_attach(s.h, fb.handle(eng), hip.FBANK_MIXED), "attach"),
                after_push=lambda s: _read_rows(s, fb.n_mels, 2))


def _read_embeddings(s, slots):
    fn = getattr(s.lib, s.names["embeddings"])
    for slot in range(slots):
        b = s.c.buffers(s.layout, {}, {"a": Out("f32", size=spec.EMB), "b": Out("f32", size=spec.EMB)})
        _ok(fn(s.h, slot, b.p("a"), b.p("b"), s.eng._stream()), s.names["embeddings"])
        b = s.c.buffers(s.layout, {}, {"b": Out("f32", size=spec.EMB)})
        _ok(fn(s.h, slot, None, b.p("b"), s.eng._stream()), s.names["embeddings"])


def test_capture_embeddings(eng):
    lib = hip.load()
    for names, opener in ((ONLINE, lambda h: lib.nhans_online_open_slots(eng.handle, 2, 0, eng._stream(), h)),
                          (LIVE, lambda h: lib.nhans_live_open_slots(eng.handle, 2, 48000, 0, 32767.0, 48000, 0, 32767.0, 0, eng._stream(), h))):
        c = Contract(eng)
        for layout in LAYOUTS:
            s = _Session(eng, c, layout, opener, names, 2, "f32", {})
            try:
                s.condition(2)
                _read_embeddings(s, 2)
            finally:
                s.close()
        runs = c.check(names["embeddings"])
        emb = _embeddings(eng).cpu().numpy()
        assert MC.same_bits(runs["A"][0][0].built["a"].buf.region()[:spec.EMB], emb[0])
        assert MC.same_bits(runs["A"][0][0].built["b"].buf.region()[:spec.EMB], emb[1])


def _live_run(eng, what, rate, kind, after_open=None, after_push=None, names=LIVE, streams=2, cin=1, cout=1, mode=None):
    """`streams` streams of 10 ms pushes at `rate` both ways, wet factor 0.25; stream 1 takes pushes of 0, 1 and 7 frames
    between whole ones and ends one push early."""
    lib = hip.load()
    rng = _rng(22)
    hop = rate // 100
    scale = 1.0 if kind == "f32" else 32767.0
    slots = streams * (cin if mode == hip.INTERLEAVED_SPLIT else 1)
    sizes = [[hop] * streams for _ in range(PUSHES)]
    for k, v in ((1, 0), (3, 1), (5, 7)):
        sizes[k][1] = v
    sizes[PUSHES - 1][1] = 0
    x = [[_pcm(rng, n * cin, kind) for n in row] for row in sizes]
    if mode is None:
        opener = lambda h: lib.nhans_live_open_slots(eng.handle, streams, rate, FORMAT[kind], 32767.0, rate, FORMAT[kind], scale,
                                                     hip.LIVE_WET, eng._stream(), h)
    else:
        opener = lambda h: lib.nhans_interleaved_live_open(eng.handle, streams, cin, cout, mode, rate, FORMAT[kind], 32767.0, rate,
                                                           FORMAT[kind], scale, hip.LIVE_WET, eng._stream(), h)
    c = Contract(eng)
    emitted = None
    for layout in LAYOUTS:
        s = _Session(eng, c, layout, opener, names, streams, kind, {"out": kind}, cin, cout)
        try:
            s.condition(slots, slots // streams)
            _ok(lib.nhans_live_set_wet(s.h, 0.25), "set_wet")
            if after_open:
                after_open(s)
            counts = []
            for k in range(PUSHES):
                counts.append(s.push(x[k], ending=[1] if k == PUSHES - 2 else ([0] if k == PUSHES - 1 else [])))
                if after_push:
                    after_push(s)
        finally:
            s.close()
        assert emitted in (None, counts)
        emitted = counts
    assert any(emitted[k][0] for k in range(1, PUSHES - 1)) and emitted[-1][0] > 0 and emitted[-2][1] > 0, emitted
    c.check(what)
    return emitted


@pytest.mark.parametrize("rate,kind", [(48000, "i16"), (44100, "f32")])
def test_live_push(eng, rate, kind):
    _live_run(eng, "nhans_live_push %d %s" % (rate, kind), rate, kind)


@pytest.mark.parametrize("mode", ["downmix", "split"])
def test_interleaved_live_push(eng, mode):
    """Offsets and counts in frames: the slack between two streams' rooms is whole frames, every channel of which stays
    sentinel; the poison around the input starts at the first element behind a stream's last frame."""
    if mode == "downmix":
        _live_run(eng, "nhans_interleaved_live_push downmix 2 -> 3", 48000, "i16", names=INTERLEAVED, cin=2, cout=3,
                  mode=hip.INTERLEAVED_DOWNMIX)
    else:
        _live_run(eng, "nhans_interleaved_live_push split 2", 48000, "i16", names=INTERLEAVED, cin=2, cout=2, mode=hip.INTERLEAVED_SPLIT)


def test_fbank_live_read(eng):
    import fbank_checks as FC
    fb = FC.bank("custom")
    _live_run(eng, "nhans_fbank_live_read", 48000, "i16",
              after_open=lambda s: _ok(s.lib.nhans_fbank_live_attach(s.h, fb.handle(eng), hip.FBANK_MIXED), "attach"),
              after_push=lambda s: _read_rows(s, fb.n_mels, 2))


def test_level_live_gains(eng):
    """A host array: room for five gains more than the push made final, the room behind the count keeps its bits."""
    lib = hip.load()
    seen = []

    def gains(s):
        for slot in range(2):
            n = lib.nhans_level_live_gains(s.h, slot, None, 0, s.eng._stream())
            assert n >= 0, lib.nhans_last_error()
            per = []
            for fill in (0x5AFEC0DE, 0x7FD5AFE5):
                host = np.full(16 + n + 5, fill, dtype=np.uint32)
                p = host[16:].ctypes.data_as(ctypes.POINTER(ctypes.c_float))
                assert lib.nhans_level_live_gains(s.h, slot, p, n + 5, s.eng._stream()) == n
                assert (host[:16] == fill).all() and (host[16 + n:] == fill).all(), "slot %d: %d gains, %s" % (slot, n, host[16 + n:])
                per.append(host[16:16 + n].copy())
            assert np.array_equal(per[0], per[1])                      # every counted gain was written
            seen.append((s.layout, slot, per[0]))

    def enable(s):
        _ok(lib.nhans_level_live_enable(s.h, s.eng._stream()), "enable")
        _ok(lib.nhans_level_live_auto(s.h, 4, 1.0), "auto")

    _live_run(eng, "nhans_level_live_gains", 48000, "i16", after_open=enable, after_push=gains)
    by = {k: [g for lay, _, g in seen if lay == k] for k in LAYOUTS}
    assert sum(len(g) for g in by["exact"]) > 0
    for k in ("A", "B"):
        assert len(by[k]) == len(by["exact"]) and all(np.array_equal(a, e) for a, e in zip(by[k], by["exact"]))


# ---- the whole-clip twin of a full-band session -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_fullband_mix(eng, kind):
    lib = hip.load()
    rate = 48000
    n16 = [0, 1, 161, 700]
    rng = _rng(23)
    den = [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in n16]
    mix = [(d + 0.05 * rng.standard_normal(len(d))).astype(np.float32) for d in den]
    counts = [resample.out_count(n, 16000, rate) for n in n16]
    x = [_pcm(rng, n, kind) for n in (counts[0], counts[1], counts[2] - 5, counts[3])]      # (a clip whose input ends early)
    hops = [rng.uniform(0.0, 1.0, -(-n // 160)).astype(np.float32) for n in n16]
    scale = 1.0 if kind == "f32" else 32767.0
    for table in (False, True):
        ins = {"x": In(kind, x), "den": In("f32", den), "mix": In("f32", mix)}
        if table:
            ins["hops"] = In("f32", hops)
        run_contract(eng, ins, {"out": Out(kind, counts)},
                     lambda b: lib.nhans_fullband_mix(eng.handle, b.p("x"), FORMAT[kind], b.o("x"), b.p("den"), b.p("mix"), b.o("den"),
                                                      len(n16), rate, 32767.0, 0.3, b.p("hops"), 1.0, scale, FORMAT[kind], b.p("out"),
                                                      b.o("out"), eng._stream()),
                     "nhans_fullband_mix %s table %d" % (kind, table), in_align=1 + table, out_align=3)


# ---- the whole hot path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_enhance_clips(eng, precision):
    """2 clips of 1 and 3 frames; the outputs that use the mixture's sample offsets have exact rooms (guards and a tail are
    watched), the context clip of 203 frames carries poison from sample 32,240 on: only its first 200 frames are read."""
    lib = hip.load()
    rng = _rng(24)
    mixes = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (400, 720)]
    T, C = 4, hip.CAPTURE_SAMPLES
    ca = [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in (C, C)]
    cb = [(0.2 * rng.standard_normal(n)).astype(np.float32) for n in (C, 480, C)]     # clip 0 = pieces 0 and 1: 203 frames
    ins = {"mix": In("f32", mixes), "ca": In("f32", ca), "cb": In("f32", cb, dead=[1])}
    total = sum(len(m) for m in mixes)
    outs = {"den": Out("f32", size=total), "mixed": Out("f32", size=total), "logmag": Out("f32", size=T * spec.BINS),
            "phase": Out("f32", size=T * spec.BINS), "logits": Out("f32", size=T * spec.BINS), "emb": Out("f32", size=4 * spec.EMB)}

    def call(b):
        o = b.offsets("cb")
        return lib.nhans_enhance_clips(eng.handle, b.p("mix"), b.o("mix"), 2, b.p("ca"), b.o("ca"), b.p("cb"), hip.i64_array([o[0], o[2], o[3]]),
                                       b.p("den"), b.p("mixed"), b.p("logmag"), b.p("phase"), b.p("logits"), b.p("emb"), eng._stream())

    _ok(lib.nhans_set_option(eng.handle, b"precision", precision), "precision")
    try:
        full = run_contract(eng, ins, outs, call, "nhans_enhance_clips precision %d" % precision)["A"][0][0]
        # each optional output NULL in turn: the others keep their bits
        for gone in ("mixed", "logmag", "phase", "logits", "emb"):
            c = Contract(eng)
            b = c.buffers("A", ins, {k: (None if k == gone else v) for k, v in outs.items()})
            _ok(call(b), "nhans_enhance_clips without %s" % gone)
            _sync()
            for k in outs:
                if k != gone:
                    f = MC.findings(b.built[k].buf, b.built[k].mask)
                    assert not f, "without %s, output %s: %s" % (gone, k, MC.report(f))
                    assert np.array_equal(b.built[k].buf.region_bits(), full.built[k].buf.region_bits()), (gone, k)
    finally:
        _ok(lib.nhans_set_option(eng.handle, b"precision", 1), "precision")
