"""Online enhancement: live recordings pushed piece by piece through nhans_online_* (include/nhans_hip.h), the output
bit for bit that of the offline path on the same normalised, trimmed samples.

OnlineEnhancer works over engine.Engine (torch device memory, the engine's current stream) and lite.LiteEngine
(torch-free, hiprt memory, the null stream).  The output contract lives in the header; out_counts() restates it in
Python so that it can be checked without a device."""
import ctypes
import warnings

import numpy as np

from . import hip, spec

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


def _capture_contexts(obj, fn, pairs, normalise, stream):
    pairs = list(pairs)
    n = len(pairs)
    slots = (ctypes.c_int * max(n, 1))(*[int(i) for i, _ in pairs])
    sides = (ctypes.c_int * max(n, 1))(*[capture_side(obj.eng.kind, w) for _, w in pairs])
    R = (ctypes.c_int64 * max(n, 1))()
    hip.check(fn(obj.handle, n, slots, sides, hip.CAPTURE_NORMALISE if normalise else 0, stream, R))
    return [int(R[k]) for k in range(n)]


def _embeddings(mem, fn, handle, i):
    rows = mem.empty(2 * spec.EMB)
    try:
        base = mem.p(rows).value
        hip.check(fn(handle, int(i), ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * spec.EMB), mem.stream()))
        out = np.array(mem.down(rows, 2 * spec.EMB), dtype=np.float32)
    finally:
        mem.free(rows)
    return out[:spec.EMB].copy(), out[spec.EMB:].copy()


class OnlineEnhancer:
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

    def _begin(self, engine, S, want_mixed):
        self.eng = engine
        self.lib = hip.load()
        self.S = S
        self.want_mixed = bool(want_mixed)
        self._torch = hasattr(engine, "_stream")
        self.handle = None
        self.pushed = [0] * S
        self.ended = [False] * S
        self._prev = None
        self._rs_in = self._rs_out = self._rs_mix = None
        self.lookahead = [LOOKAHEAD] * S

    def _lookaheads(self, lookahead):
        la = list(lookahead) if hasattr(lookahead, "__len__") else [lookahead] * self.S
        if len(la) != self.S:
            raise ValueError("lookahead: one value, or one per slot (%d)" % self.S)
        for i, L in enumerate(la):
            if L != LOOKAHEAD:
                self.set_lookahead(i, L)

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
        self._begin(engine, len(ctx_a), want_mixed)
        self.conditioned = [True] * self.S
        a, aoff = self._flat(ctx_a)
        b, boff = self._flat(ctx_b)
        da, db = self._up(a), self._up(b)
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_online_open(engine.handle, self.S, self._p(da), hip.i64_array(aoff), self._p(db),
                                             hip.i64_array(boff), int(self.want_mixed), self._stream(), ctypes.byref(h)))
        self.handle = h
        self._free(da, db)
        self._rates(in_rate, out_rate, peak, in_dtype)
        self._lookaheads(lookahead)

    @classmethod
    def open_slots(cls, engine, nslots, want_mixed=False, in_rate=None, out_rate=None, peak=None, in_dtype=np.int16,
                   lookahead=LOOKAHEAD):
        """An object of nslots unconditioned slots (nhans_online_open_slots): no tower runs until a set_context."""
        self = cls.__new__(cls)
        self._begin(engine, int(nslots), want_mixed)
        self.conditioned = [False] * self.S
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_online_open_slots(engine.handle, self.S, int(self.want_mixed), self._stream(), ctypes.byref(h)))
        self.handle = h
        self._rates(in_rate, out_rate, peak, in_dtype)
        self._lookaheads(lookahead)
        return self

    # ---- device memory of either engine --------------------------------------------------------
    @staticmethod
    def _flat(arrays):
        off = [0]
        for x in arrays:
            off.append(off[-1] + len(x))
        flat = np.concatenate([np.asarray(x, dtype=np.float32) for x in arrays]) if len(arrays) else np.zeros(0, np.float32)
        return np.ascontiguousarray(flat, dtype=np.float32), off

    def _stream(self):
        return self.eng._stream() if self._torch else None

    def _up(self, arr):
        if self._torch:
            import torch
            return torch.from_numpy(arr).to(self.eng.device)
        from . import hiprt
        return hiprt.DevBuf.from_array(arr)

    def _empty(self, n):
        if self._torch:
            import torch
            return torch.empty(max(n, 1), dtype=torch.float32, device=self.eng.device)
        from . import hiprt
        return hiprt.DevBuf(4 * max(n, 1))

    def _p(self, buf):
        return hip.ptr(buf) if self._torch else buf.ptr

    def _down(self, buf, n):
        if self._torch:
            return buf[:n].cpu().numpy()
        return buf.to_array(np.empty(n, np.float32)) if n else np.zeros(0, np.float32)

    def _free(self, *bufs):
        if not self._torch:
            for b in bufs:
                if b is not None:
                    b.free()

    def _set_precision(self, p):
        if hasattr(self.eng, "set_precision"):
            self.eng.set_precision(p)
        else:
            self.eng.set_option("precision", {"f32": 0, "f16x3": 1}[p])

    # ---- the C ABI ---------------------------------------------------------------------------
    def out_counts(self, counts, end=None):
        """nhans_online_out_counts: what a push of counts[i] samples would emit per stream."""
        out = (ctypes.c_int64 * self.S)()
        endv = (ctypes.c_int * self.S)(*[int(bool(e)) for e in end]) if end is not None else None
        hip.check(self.lib.nhans_online_out_counts(self.handle, hip.i64_array(counts), endv, out))
        return list(out)

    def rewind(self):
        hip.check(self.lib.nhans_online_rewind(self.handle))
        self.pushed, self.ended = self._prev

    def restart(self, i):
        """Slot i becomes an open stream of 0 samples (nhans_online_restart); conditioning is kept."""
        hip.check(self.lib.nhans_online_restart(self.handle, int(i)))
        self.pushed[i], self.ended[i] = 0, False
        for rs in (self._rs_in, self._rs_out, self._rs_mix):
            if rs is not None:
                rs.restart(i)

    def set_lookahead(self, i, L):
        """The look-ahead of slot i, L frames in 0 .. 17 (nhans_online_set_lookahead): allowed while the slot's stream has
        no samples yet -- after open or restart(i) --, kept across restarts."""
        L = spec.check_lookahead(L)
        hip.check(self.lib.nhans_online_set_lookahead(self.handle, int(i), L))
        self.lookahead[i] = L

    def first_new_frame(self, i):
        """R of slot i: the frames of its stream already computed, which a change of conditioning leaves as they are."""
        return ready_frames(self.pushed[i], self.ended[i], self.lookahead[i])

    def set_context(self, i, ctx_a, ctx_b):
        """Conditions slot i on two recordings (nhans_online_set_context).  Returns R: frames >= R of the slot's stream
        use the new conditioning (change_bounds(R) for what that means in samples)."""
        a = np.ascontiguousarray(ctx_a, dtype=np.float32)
        b = np.ascontiguousarray(ctx_b, dtype=np.float32)
        da, db = self._up(a), self._up(b)
        R = ctypes.c_int64(-1)
        try:
            hip.check(self.lib.nhans_online_set_context(self.handle, int(i), self._p(da), len(a), self._p(db), len(b),
                                                        self._stream(), ctypes.byref(R)))
        finally:
            self._free(da, db)
        self.conditioned[i] = True
        return int(R.value)

    def set_embeddings(self, i, emb_a, emb_b):
        """The same with two ready [512] rows (Engine.embed; host arrays or, over Engine, device tensors)."""
        rows = []
        for e in (emb_a, emb_b):
            if self._torch and hasattr(e, "data_ptr"):
                import torch
                e = e.detach().to(device=self.eng.device, dtype=torch.float32).contiguous().reshape(-1)
            else:
                e = self._up(np.ascontiguousarray(e, dtype=np.float32).reshape(-1))
            rows.append(e)
        n = [r.numel() if hasattr(r, "numel") else r.nbytes // 4 for r in rows]
        if n != [spec.EMB, spec.EMB]:
            self._free(*[r for r in rows if not hasattr(r, "numel")])
            raise ValueError("set_embeddings: two rows of %d floats" % spec.EMB)
        R = ctypes.c_int64(-1)
        try:
            hip.check(self.lib.nhans_online_set_embeddings(self.handle, int(i), self._p(rows[0]), self._p(rows[1]),
                                                           self._stream(), ctypes.byref(R)))
        finally:
            self._free(*[r for r in rows if not hasattr(r, "numel")])
        self.conditioned[i] = True
        return int(R.value)

    # ---- conditioning captured from the slot's own stream -------------------------------------
    def enable_capture(self):
        """Every slot gets its sample history (nhans_capture_enable; idempotent): pushes from now on feed it."""
        hip.check(self.lib.nhans_capture_enable(self.handle, self._stream()))

    def capture_contexts(self, pairs, normalise=True):
        """pairs: [(slot, which), ...], which 'a' / 'b' / 'neg' / 'pos' (capture_side).  Each slot's row `which` becomes
        the embedding of the last CAPTURE_SAMPLES samples of its own stream (peak-normalised as apply.normalise does, or as
        stored); one tower pass for all of them.  Returns [R, ...] as set_context does.  NhansError with .code ==
        hip.ESHORT where capture_span is None."""
        return _capture_contexts(self, self.lib.nhans_capture_context, pairs, normalise, self._stream())

    def capture_context(self, i, which, normalise=True):
        return self.capture_contexts([(i, which)], normalise)[0]

    def embeddings(self, i):
        """(a, b): slot i's current conditioning rows as two float32[512] arrays (nhans_capture_embeddings) -- a learnt
        noise profile that set_embeddings accepts elsewhere."""
        from . import resample
        return _embeddings(resample._Mem(self.eng), self.lib.nhans_capture_embeddings, self.handle, i)

    def _push_once(self, din, inoff, endv, counts):
        ooff = [0]
        for n in counts:
            ooff.append(ooff[-1] + n)
        dden = self._empty(ooff[-1])
        dmix = self._empty(ooff[-1]) if self.want_mixed else None
        got = (ctypes.c_int64 * self.S)()
        hip.check(self.lib.nhans_online_push(self.handle, self._p(din), hip.i64_array(inoff), endv, self._p(dden),
                                             self._p(dmix) if dmix is not None else None, hip.i64_array(ooff), got,
                                             self._stream()))
        return dden, dmix, ooff, list(got)

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
        flat, inoff = self._flat(chunks)
        counts = [inoff[i + 1] - inoff[i] for i in range(self.S)]
        endv = (ctypes.c_int * self.S)(*[int(bool(e)) for e in end]) if end is not None else None
        outc = self.out_counts(counts, end)
        din = self._up(flat)
        dden, dmix, ooff, got = self._push_once(din, inoff, endv, outc)
        self._prev = (list(self.pushed), list(self.ended))
        if self.eng.take_status() & hip.STATUS_SATURATED and self.eng.precision == "f16x3":
            warnings.warn("N-HANS f16x3 path: an activation left the f16 range; batch recomputed in f32 MFMA mode "
                          "and the activation exponents raised")
            hip.check(self.lib.nhans_online_rewind(self.handle))
            self._free(dden, dmix)
            self.eng.set_option("calibrate", 1)
            try:
                self._set_precision("f32")
                dden, dmix, ooff, got = self._push_once(din, inoff, endv, outc)
                self.eng.take_status()
            except BaseException:
                try:
                    self.eng.set_option("calibrate", 3)
                finally:
                    self._set_precision("f16x3")
                raise
            try:
                self.eng.set_option("calibrate", 2)
            except hip.NhansError as err:
                warnings.warn("N-HANS: activation exponents not updated after the f32 rerun: %s" % err)
            finally:
                self._set_precision("f16x3")
        assert got == outc, (got, outc)
        den = self._down(dden, ooff[-1])
        mix = self._down(dmix, ooff[-1]) if dmix is not None else None
        self._free(din, dden, dmix)
        for i in range(self.S):
            self.pushed[i] += counts[i]
            self.ended[i] = self.ended[i] or bool(end is not None and end[i])
        return [(den[ooff[i]:ooff[i + 1]], mix[ooff[i]:ooff[i + 1]] if mix is not None else None) for i in range(self.S)]

    def close(self):
        for name in ("_rs_in", "_rs_out", "_rs_mix"):
            rs = getattr(self, name, None)
            if rs is not None:
                rs.close()
                setattr(self, name, None)
        if getattr(self, "handle", None):
            self.lib.nhans_online_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
