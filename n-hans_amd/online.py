"""Online enhancement: live recordings pushed piece by piece through nhans_online_* (include/nhans_hip.h), the output
bit for bit that of the offline path on the same normalised, trimmed samples.

OnlineEnhancer works over engine.Engine (torch device memory, the engine's current stream) and lite.LiteEngine
(torch-free, hiprt memory, the null stream).  The output contract lives in the header; out_counts() restates it in
Python so that it can be checked without a device."""
import ctypes

import numpy as np

from . import context, hip, spec

LOOKAHEAD = spec.MIX_WIN // 2          # 17 frames


def num_frames(n):
    return 0 if n < spec.WIN else 1 + (n - spec.WIN) // spec.HOP


def ready_frames(n, ended, lookahead=LOOKAHEAD):
    """R of the header's contract: the frames of a stream of n pushed samples that are computed -- those whose
    `lookahead` future rows exist, all of them once the stream has ended."""
    T = num_frames(n)
    return T if ended else max(0, T - lookahead)


def emitted(n, ended, lookahead=LOOKAHEAD):
    """Samples a stream of n pushed samples has emitted in total (include/nhans_hip.h: the output contract): 160 * P with
    P = R rounded down to even, R = ready_frames; the offline length once ended."""
    T = num_frames(n)
    if ended:
        return 0 if T == 0 else (T - 1) * spec.HOP + spec.WIN
    R = max(0, T - lookahead)
    return spec.HOP * (R - R % 2)


def out_counts(n_before, n_push, end=None, ended_before=None, lookahead=LOOKAHEAD):
    """Per-stream sample counts a push of n_push[i] samples (end[i]: the stream ends after them) reports, for streams
    that had n_before[i] samples (ended_before[i]: and had ended) -- what nhans_online_out_counts computes.  lookahead:
    one L for all streams, or one per stream."""
    S = len(n_before)
    end = end if end is not None else [False] * S
    ended_before = ended_before if ended_before is not None else [False] * S
    la = list(lookahead) if hasattr(lookahead, "__len__") else [lookahead] * S
    return [emitted(n_before[i] + n_push[i], bool(end[i] or ended_before[i]), la[i])
            - emitted(n_before[i], bool(ended_before[i]), la[i]) for i in range(S)]


def change_bounds(R):
    """(last_old_sample_excl, first_new_sample) of a change of conditioning that reported first frame R (include/
    nhans_hip.h, the mid-stream contract): output samples below the first are bit for bit the offline output under the
    old conditioning, samples from the second on that under the new one.  The iSTFT transforms frames in pairs
    (2k, 2k+1), so the old side stops at the pair that holds frame R and the new side starts after it, one window
    overlap (400 - 160) later.  R = 0 and R = the final frame count are whole-output cases the caller knows about.
    R is ready_frames(n, ended, L) of the slot at the time of the change -- T - L for a running stream of look-ahead L --,
    and "the offline output" is that of the same L (Engine.enhance(..., lookahead=L))."""
    return spec.HOP * (R - R % 2), spec.HOP * (R + R % 2) + spec.WIN - spec.HOP


def latency_ms(fs=spec.FS, in_rate=None, out_rate=None, lookahead=LOOKAHEAD):
    """Algorithmic latency (ms) from a sample's arrival to its output: the look-ahead of `lookahead` frames plus one
    window, less or more one hop for where the sample falls in its hop and for the even-pair rule of the iSTFT:
    10 L + 25 +- 10 ms at 16 kHz -> (185, 205) at the default 17, (35, 55) at 2, (15, 35) at 0.
    in_rate / out_rate: plus the filter delay of each rate conversion (resample.latency_ms: 0.625 ms beside 16 kHz)."""
    mid = (lookahead * spec.HOP + spec.WIN) * 1000.0 / fs
    if in_rate is not None or out_rate is not None:
        from . import resample
        mid += resample.latency_ms(in_rate, fs) if in_rate is not None else 0.0
        mid += resample.latency_ms(fs, out_rate) if out_rate is not None else 0.0
    return mid - spec.HOP * 1000.0 / fs, mid + spec.HOP * 1000.0 / fs


def normalise_fixed(samples, peak):
    """samples / (peak + 1e-6) in float64 -> float32: apply.normalise with a peak the live caller picks (dividing, not
    multiplying by a gain: the rounding is that of the offline normalisation when peak = max|x|)."""
    return (np.asarray(samples, dtype=np.float64) / (peak + 0.000001)).astype(np.float32)


CAPTURE_SAMPLES = hip.CAPTURE_SAMPLES      # 32,240 = 199 * 160 + 400: the 200 context frames


def ring_runs(n_before, count):
    """nhans_capture_plan restated: the copy runs (offset in the push, ring position, length) that append `count` samples
    to a slot's ring of CAPTURE_SAMPLES floats which has seen n_before -- sample k of the stream goes to position
    k mod CAPTURE_SAMPLES, only the last CAPTURE_SAMPLES of a larger push are kept, at most two runs, none for count 0."""
    if n_before < 0 or count < 0:
        raise ValueError("ring_runs: negative sample count")
    if count == 0:
        return []
    skip = max(0, count - CAPTURE_SAMPLES)
    n = count - skip
    pos = (n_before + skip) % CAPTURE_SAMPLES
    first = min(n, CAPTURE_SAMPLES - pos)
    runs = [(skip, pos, first)]
    if first < n:
        runs.append((skip + first, 0, n - first))
    return runs


def capture_vlo(vlo, event, n):
    """vlo of a slot -- the oldest sample of its current stream that the ring still holds (include/nhans_hip.h) -- after
    `event`: 'enable' (n: the slot's sample count then) -> n; 'restart' -> 0; 'push' (n: the count the push reached) and
    'rewind' (n: the count the UNDONE push had reached; its samples stay in the ring) -> max(vlo, n - CAPTURE_SAMPLES)."""
    if event == "enable":
        return n
    if event == "restart":
        return 0
    if event in ("push", "rewind"):
        return max(vlo, n - CAPTURE_SAMPLES)
    raise ValueError("capture_vlo: event %r" % (event,))


def capture_span(n_pushed_16k, vlo):
    """(first, last + 1) of the 16 kHz samples a capture would take from a slot that has received n_pushed_16k samples and
    whose ring holds its stream from sample vlo on -- or None where the library answers NHANS_ESHORT: too few samples yet,
    history enabled too recently, a rewound push not yet repeated."""
    lo = n_pushed_16k - CAPTURE_SAMPLES
    return (lo, n_pushed_16k) if lo >= vlo else None


def capture_side(kind, which):
    """'a' / 'b' / 'neg' / 'pos' -> NHANS_CAPTURE_A / _B.  'neg' and 'pos' follow the model kind as the header defines the
    (a, b) order: denoiser a = pos, b = neg; separator a = neg (the interferer), b = pos (the target)."""
    if which in (hip.CAPTURE_A, "a"):
        return hip.CAPTURE_A
    if which in (hip.CAPTURE_B, "b"):
        return hip.CAPTURE_B
    if which in ("neg", "pos") and kind in hip.KIND_CODE:
        a_is = "pos" if hip.KIND_CODE[kind] == hip.DENOISER else "neg"
        return hip.CAPTURE_A if which == a_is else hip.CAPTURE_B
    raise ValueError("which: 'a', 'b', 'neg' or 'pos' (got %r for a %s)" % (which, kind))


class Slots:
    """What OnlineEnhancer and live.LiveSession share: S slots that outlive their streams (include/nhans_hip.h, "Slots")
    behind one C object `handle` over the context `eng`.  C names the object's entry points -- spelt out, the two
    families are not named alike -- and they are looked up when called: a library from before a feature ($NHANS_LIB)
    lacks its symbols, and only using the feature is an error."""

    C = {}
    handle = None

    def _begin(self, engine, S, conditioned):
        self.eng = engine
        self.mem = context.Mem(engine)
        self.lib = hip.load()
        self.S = int(S)
        self.handle = None
        self.pushed = [0] * self.S
        self.ended = [False] * self.S
        self.conditioned = [conditioned] * self.S
        self._prev = None
        self._fbank_n = 0
        self.lookahead = [LOOKAHEAD] * self.S

    def _c(self, what, *args):
        return hip.check(getattr(self.lib, self.C[what])(self.handle, *args))

    def _lookaheads(self, lookahead):
        la = list(lookahead) if hasattr(lookahead, "__len__") else [lookahead] * self.S
        if len(la) != self.S:
            raise ValueError("lookahead: one value, or one per slot (%d)" % self.S)
        for i, L in enumerate(la):
            if L != LOOKAHEAD:
                self.set_lookahead(i, L)

    def out_counts(self, counts, end=None):
        """What a push of counts[i] samples would emit per slot."""
        out = (ctypes.c_int64 * self.S)()
        self._c("out_counts", hip.i64_array(counts), context.end_flags(end, self.S), out)
        return list(out)

    def rewind(self):
        self._c("rewind")
        self.pushed, self.ended = self._prev

    def restart(self, i):
        """Slot i becomes an open stream of 0 samples, in every stage; conditioning is kept."""
        self._c("restart", int(i))
        self.pushed[i], self.ended[i] = 0, False

    def set_lookahead(self, i, L):
        """The look-ahead of slot i, L frames in 0 .. 17: allowed while the slot's stream has no samples yet -- after open
        or restart(i) --, kept across restarts."""
        L = spec.check_lookahead(L)
        self._c("set_lookahead", int(i), L)
        self.lookahead[i] = L

    def set_context(self, i, ctx_a, ctx_b):
        """Conditions slot i on two normalised 16 kHz recordings.  Returns R: frames >= R of the slot's 16 kHz stream use
        the new conditioning (change_bounds(R) for what that means in samples)."""
        a = np.ascontiguousarray(ctx_a, dtype=np.float32)
        b = np.ascontiguousarray(ctx_b, dtype=np.float32)
        da, db = self.mem.up(a), self.mem.up(b)
        R = ctypes.c_int64(-1)
        try:
            self._c("set_context", int(i), self.mem.p(da), len(a), self.mem.p(db), len(b), self.mem.stream(), ctypes.byref(R))
        finally:
            self.mem.free(da, db)
        self.conditioned[i] = True
        return int(R.value)

    def set_embeddings(self, i, emb_a, emb_b):
        """The same with two ready [512] rows (Engine.embed; host arrays or, over Engine, device tensors)."""
        rows, own = [], []
        R = ctypes.c_int64(-1)
        try:
            for e in (emb_a, emb_b):
                buf, n, ours = self.mem.up_f32(e)
                if ours:
                    own.append(buf)
                if n != spec.EMB:
                    raise ValueError("set_embeddings: two rows of %d floats" % spec.EMB)
                rows.append(buf)
            self._c("set_embeddings", int(i), self.mem.p(rows[0]), self.mem.p(rows[1]), self.mem.stream(), ctypes.byref(R))
        finally:
            self.mem.free(*own)       # (what was uploaded here; a caller's tensor stays the caller's)
        self.conditioned[i] = True
        return int(R.value)

    # ---- conditioning captured from the slot's own stream -------------------------------------
    def enable_capture(self):
        """Every slot gets its 16 kHz sample history (idempotent): pushes from now on feed it."""
        self._c("capture_enable", self.mem.stream())

    def capture_contexts(self, pairs, normalise=True):
        """pairs: [(slot, which), ...], which 'a' / 'b' / 'neg' / 'pos' (capture_side).  Each slot's row `which` becomes
        the embedding of the last CAPTURE_SAMPLES samples of its own 16 kHz stream -- with an incoming rate, of what the
        converter handed on -- (peak-normalised as apply.normalise does, or as stored); one tower pass for all of them.
        Returns [R, ...] as set_context does.  NhansError with .code == hip.ESHORT where capture_span is None."""
        pairs = list(pairs)
        n = len(pairs)
        slots = (ctypes.c_int * max(n, 1))(*[int(i) for i, _ in pairs])
        sides = (ctypes.c_int * max(n, 1))(*[capture_side(self.eng.kind, w) for _, w in pairs])
        R = (ctypes.c_int64 * max(n, 1))()
        self._c("capture_context", n, slots, sides, hip.CAPTURE_NORMALISE if normalise else 0, self.mem.stream(), R)
        return [int(R[k]) for k in range(n)]

    def capture_context(self, i, which, normalise=True):
        return self.capture_contexts([(i, which)], normalise)[0]

    def embeddings(self, i):
        """(a, b): slot i's current conditioning rows as two float32[512] arrays -- a learnt noise profile that
        set_embeddings accepts elsewhere."""
        rows = self.mem.empty(2 * spec.EMB)
        try:
            base = self.mem.p(rows).value
            self._c("capture_embeddings", int(i), ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * spec.EMB), self.mem.stream())
            out = np.array(self.mem.down(rows, 2 * spec.EMB), dtype=np.float32)
        finally:
            self.mem.free(rows)
        return out[:spec.EMB].copy(), out[spec.EMB:].copy()

    # ---- filterbank features of the frames a push computes (include/nhans_hip.h: nhans_fbank_*) -
    def enable_fbank(self, fb, mixed=False):
        """From the next push on, every push also computes fb (fbank.Filterbank) of the frames it computes -- one small
        launch more --, for features(i) to read; mixed=True: also of the same frames' unprocessed rows (plane 1).  The
        table is copied into the object: fb may be closed.  None detaches.  The rows of the last push are voided."""
        self._c("fbank_attach", fb.handle(self.eng) if fb is not None else None,
                hip.FBANK_MIXED if (fb is not None and mixed) else 0)
        self._fbank_n = fb.n_mels if fb is not None else 0

    def features(self, i, plane=0):
        """(first_frame, float32 [rows, n_mels]): the feature rows the most recent push computed for slot i -- frames
        first_frame .. of its 16 kHz stream, frame g centred on sample 160 g + 200; ready_frames() says which frames a
        push computes.  plane 1: the unprocessed rows (enable_fbank(mixed=True)).  No rows after rewind(), restart(i),
        enable_fbank or for a slot the push computed nothing for; a push redone after saturation brings the redone rows."""
        first = ctypes.c_int64(-1)
        n = self._c("fbank_read", int(i), int(plane), None, 0, ctypes.byref(first), self.mem.stream())
        nm = self._fbank_n
        if n == 0:
            return int(first.value), np.zeros((0, nm), dtype=np.float32)
        buf = self.mem.empty(n * nm)
        try:
            self._c("fbank_read", int(i), int(plane), self.mem.p(buf), n, ctypes.byref(first), self.mem.stream())
            out = np.array(self.mem.down(buf, n * nm), dtype=np.float32).reshape(n, nm)
        finally:
            self.mem.free(buf)
        return int(first.value), out

    def _push_checked(self, push, counts, end, outc):
        """push(): one call of the push entry point, returning the counts it reported.  A push that saturates the f16x3
        path is undone and redone in f32 (context.redo_saturated_in_f32); then the host's view of the slots moves on."""
        def run():
            got = push()
            self._prev = (list(self.pushed), list(self.ended))
            return got

        got = context.redo_saturated_in_f32(self.eng, run, lambda: self._c("rewind"))
        assert got == outc, (got, outc)
        for i in range(self.S):
            self.pushed[i] += counts[i]
            self.ended[i] = self.ended[i] or bool(end is not None and end[i])

    def close(self):
        if self.handle:
            getattr(self.lib, self.C["close"])(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OnlineEnhancer(Slots):
    """S live recordings conditioned on ctx_a[i] / ctx_b[i] (normalised float32, >= 32,240 samples each; resnet_block
    argument order as everywhere: denoiser (pos, neg), separator (noise, clean)).

    The S positions are slots that outlive their streams (include/nhans_hip.h, "Slots"): open_slots() makes an object of
    unconditioned slots, restart(i) + set_context(i, a, b) lets a new recording join in slot i, end in a push or
    restart(i) lets it leave, set_context / set_embeddings alone change the conditioning of a running stream.

    in_rate / out_rate (Hz, resample.RATES): push() then takes pieces at in_rate -- in_dtype int16 or float32; peak: every
    converted sample is divided by (peak + 1e-6) on the device, normalise_fixed -- and returns pieces at out_rate, each
    through a resample.Resampler of its own (a second outgoing one for the mixed round trip).  The output is bit for bit
    resample -> normalise_fixed -> offline enhance -> resample of the whole recording.  With both None the object is
    the 16 kHz one and none of this exists.

    lookahead: L frames, 0 .. 17, one for all slots or one per slot (set_lookahead(i, L) later, on a slot whose stream
    has no samples yet).  The output is then bit for bit the offline one of that L: Engine.enhance(..., lookahead=L).

    enable_capture() + capture_context(i, which): slot i's conditioning, side `which`, taken from the last 2.015 s the
    slot itself has received at 16 kHz (include/nhans_hip.h, "Conditioning captured from a slot's own stream") -- with
    in_rate, from what the incoming converter handed on."""

    C = dict(restart="nhans_online_restart", rewind="nhans_online_rewind", out_counts="nhans_online_out_counts",
             set_context="nhans_online_set_context", set_embeddings="nhans_online_set_embeddings",
             set_lookahead="nhans_online_set_lookahead", capture_enable="nhans_capture_enable",
             capture_context="nhans_capture_context", capture_embeddings="nhans_capture_embeddings",
             fbank_attach="nhans_fbank_online_attach", fbank_read="nhans_fbank_online_read", close="nhans_online_close")

    def _begin(self, engine, S, conditioned, want_mixed):
        super()._begin(engine, S, conditioned)
        self.want_mixed = bool(want_mixed)
        self._rs_in = self._rs_out = self._rs_mix = None

    def _rates(self, in_rate, out_rate, peak, in_dtype):
        if in_rate is None and out_rate is None:
            if peak is not None:
                raise ValueError("peak= normalises the converted input: it needs in_rate")
            return
        from . import resample
        if in_rate is not None:
            self._rs_in = resample.Resampler(self.eng, self.S, in_rate, spec.FS, dtype=in_dtype, peak=peak)
        elif peak is not None:
            raise ValueError("peak= normalises the converted input: it needs in_rate")
        if out_rate is not None:
            self._rs_out = resample.Resampler(self.eng, self.S, spec.FS, out_rate)
            if self.want_mixed:
                self._rs_mix = resample.Resampler(self.eng, self.S, spec.FS, out_rate)

    def __init__(self, engine, ctx_a, ctx_b, want_mixed=False, in_rate=None, out_rate=None, peak=None, in_dtype=np.int16,
                 lookahead=LOOKAHEAD):
        if len(ctx_a) != len(ctx_b):
            raise ValueError("ctx_a and ctx_b must have one recording per stream")
        self._begin(engine, len(ctx_a), True, want_mixed)
        a, aoff = context.flat(ctx_a)
        b, boff = context.flat(ctx_b)
        da, db = self.mem.up(a), self.mem.up(b)
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_online_open(engine.handle, self.S, self.mem.p(da), hip.i64_array(aoff), self.mem.p(db),
                                             hip.i64_array(boff), int(self.want_mixed), self.mem.stream(), ctypes.byref(h)))
        self.handle = h
        self.mem.free(da, db)
        self._rates(in_rate, out_rate, peak, in_dtype)
        self._lookaheads(lookahead)

    @classmethod
    def open_slots(cls, engine, nslots, want_mixed=False, in_rate=None, out_rate=None, peak=None, in_dtype=np.int16,
                   lookahead=LOOKAHEAD):
        """An object of nslots unconditioned slots (nhans_online_open_slots): no tower runs until a set_context."""
        self = cls.__new__(cls)
        self._begin(engine, nslots, False, want_mixed)
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_online_open_slots(engine.handle, self.S, int(self.want_mixed), self.mem.stream(),
                                                   ctypes.byref(h)))
        self.handle = h
        self._rates(in_rate, out_rate, peak, in_dtype)
        self._lookaheads(lookahead)
        return self

    def restart(self, i):
        super().restart(i)
        for rs in (self._rs_in, self._rs_out, self._rs_mix):
            if rs is not None:
                rs.restart(i)

    def first_new_frame(self, i):
        """R of slot i: the frames of its stream already computed, which a change of conditioning leaves as they are."""
        return ready_frames(self.pushed[i], self.ended[i], self.lookahead[i])

    def push(self, chunks, end=None):
        """chunks: one 1-D float32 array per stream (may be empty); end[i]: stream i ends after its chunk.  Returns
        [(denoised, mixed)] per stream -- the samples that became final (mixed is None without want_mixed).  A push
        that saturates the f16x3 path is undone and redone in f32 inside a calibrate bracket, as Engine.enhance does
        for a batch.  With in_rate / out_rate the chunks are pieces at in_rate and the results pieces at out_rate; the
        outgoing converters see only the final result of a push."""
        if self._rs_in is None and self._rs_out is None:
            return self._push16(chunks, end)
        if len(chunks) != self.S:
            raise ValueError("push: one chunk per stream (%d)" % self.S)
        res = self._push16(self._rs_in.push(chunks, end) if self._rs_in is not None else chunks, end)
        if self._rs_out is None:
            return res
        den = self._rs_out.push([d for d, _ in res], end)
        mix = self._rs_mix.push([m for _, m in res], end) if self._rs_mix is not None else [None] * self.S
        return list(zip(den, mix))

    def _push16(self, chunks, end=None):
        if len(chunks) != self.S:
            raise ValueError("push: one chunk per stream (%d)" % self.S)
        x, inoff = context.flat(chunks)
        counts = [inoff[i + 1] - inoff[i] for i in range(self.S)]
        outc = self.out_counts(counts, end)
        ooff = context.offsets(outc)
        mem = self.mem
        din, dden = mem.up(x), mem.empty(ooff[-1])
        dmix = mem.empty(ooff[-1]) if self.want_mixed else None

        def push():
            got = (ctypes.c_int64 * self.S)()
            hip.check(self.lib.nhans_online_push(self.handle, mem.p(din), hip.i64_array(inoff), context.end_flags(end, self.S),
                                                 mem.p(dden), mem.p(dmix), hip.i64_array(ooff), got, mem.stream()))
            return list(got)

        self._push_checked(push, counts, end, outc)
        den = mem.down(dden, ooff[-1])
        mix = mem.down(dmix, ooff[-1]) if dmix is not None else None
        mem.free(din, dden, dmix)
        return [(den[ooff[i]:ooff[i + 1]], mix[ooff[i]:ooff[i + 1]] if mix is not None else None) for i in range(self.S)]

    def close(self):
        for name in ("_rs_in", "_rs_out", "_rs_mix"):
            rs = getattr(self, name, None)
            if rs is not None:
                rs.close()
                setattr(self, name, None)
        super().close()
