"""Live PCM sessions (include/nhans_hip.h: nhans_live_*): pieces at the capture device's rate and format go in, pieces at
the playback device's rate and format come out, one C call per push -- rate conversion in, online enhancement, wet/dry
mix, rate conversion and PCM rounding out, with nothing on the host between the stages.  The output is bit for bit the
offline chain resample -> normalise_fixed -> trim -> enhance -> mix -> resample -> scale -> round.

LiveSession works over engine.Engine (torch device memory, the engine's current stream) and lite.LiteEngine (torch-free,
hiprt memory, the null stream).  emitted() restates the output contract of the header in Python so that it can be checked
without a device."""
import ctypes
import warnings

import numpy as np

from . import hip, online, resample, spec


def emitted(n, ended, in_rate, out_rate, lookahead=online.LOOKAHEAD):
    """Samples at out_rate a stream of n pushed samples at in_rate has emitted in total: the three stages' contracts
    chained (resample.emitted, online.emitted at the slot's look-ahead, resample.emitted)."""
    for r in (in_rate, out_rate):
        if r not in resample.RATES:
            raise ValueError("%d Hz in / %d Hz out is not supported (each one of %s)"
                             % (in_rate, out_rate, ", ".join(str(v) for v in resample.RATES)))
    n16 = resample.emitted(n, ended, in_rate, spec.FS)
    return resample.emitted(online.emitted(n16, ended, lookahead), ended, spec.FS, out_rate)


def default_out_scale(peak, out_dtype):
    """peak + 1e-6 for int16 output -- the inverse of the incoming normalisation, so that an untouched signal comes back
    on the scale it arrived on --, 1.0 for float32."""
    return float(peak) + 0.000001 if np.dtype(out_dtype) == np.int16 else 1.0


class LiveSession:
    """nslots live recordings at in_rate (in_dtype int16 or float32, every converted sample divided by peak + 1e-6) ->
    pieces at out_rate as out_dtype (int16: rounded and clipped; float32), each 16 kHz result multiplied by out_scale.
    wet=True opens the object with the mixed round trip so that set_wet(w) can blend it in:
    denoised + (mixed - denoised) * w, the reference's --compensate mix.

    Slots are the online object's (online.OnlineEnhancer): all start unconditioned; restart(i) + set_context(i, a, b)
    lets a recording join in slot i, end in a push or restart(i) lets it leave.

    lookahead: L frames, 0 .. 17, one for all slots or one per slot (set_lookahead(i, L) later, on a slot whose stream
    has no samples yet): the 16 kHz stage then computes the offline output of that L, Engine.enhance(..., lookahead=L)."""

    def __init__(self, engine, nslots, in_rate, out_rate, peak, in_dtype=np.int16, out_dtype=np.int16, out_scale=None,
                 wet=False, lookahead=online.LOOKAHEAD):
        emitted(0, False, in_rate, out_rate)
        self.mem = resample._Mem(engine)
        self.eng = engine
        self.lib = hip.load()
        self.S = int(nslots)
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.in_dtype, self.out_dtype = np.dtype(in_dtype), np.dtype(out_dtype)
        self.peak = float(peak)
        self.out_scale = default_out_scale(peak, out_dtype) if out_scale is None else float(out_scale)
        self.has_wet = bool(wet)
        self.handle = None
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_live_open_slots(engine.handle, self.S, self.in_rate, resample._format(self.in_dtype),
                                                 self.peak, self.out_rate, resample._format(self.out_dtype), self.out_scale,
                                                 hip.LIVE_WET if self.has_wet else 0, self.mem.stream(), ctypes.byref(h)))
        self.handle = h
        self.pushed = [0] * self.S
        self.ended = [False] * self.S
        self.conditioned = [False] * self.S
        self._prev = None
        self.lookahead = [online.LOOKAHEAD] * self.S
        la = list(lookahead) if hasattr(lookahead, "__len__") else [lookahead] * self.S
        if len(la) != self.S:
            raise ValueError("lookahead: one value, or one per slot (%d)" % self.S)
        for i, L in enumerate(la):
            if L != online.LOOKAHEAD:
                self.set_lookahead(i, L)

    # ---- slots ---------------------------------------------------------------------------------
    def restart(self, i):
        """Slot i becomes an open stream of 0 samples in every stage (nhans_live_restart); conditioning is kept."""
        hip.check(self.lib.nhans_live_restart(self.handle, int(i)))
        self.pushed[i], self.ended[i] = 0, False

    def set_context(self, i, ctx_a, ctx_b):
        """Conditions slot i on two normalised 16 kHz recordings (nhans_live_set_context).  Returns R: frames >= R of
        the slot's 16 kHz stream use the new conditioning (online.change_bounds)."""
        a = np.ascontiguousarray(ctx_a, dtype=np.float32)
        b = np.ascontiguousarray(ctx_b, dtype=np.float32)
        da, db = self.mem.up(a), self.mem.up(b)
        R = ctypes.c_int64(-1)
        try:
            hip.check(self.lib.nhans_live_set_context(self.handle, int(i), self.mem.p(da), len(a), self.mem.p(db), len(b),
                                                      self.mem.stream(), ctypes.byref(R)))
        finally:
            self.mem.free(da, db)
        self.conditioned[i] = True
        return int(R.value)

    def set_embeddings(self, i, emb_a, emb_b):
        """The same with two ready [512] rows (Engine.embed; host arrays or, over Engine, device tensors)."""
        rows, own = [], []
        for e in (emb_a, emb_b):
            if self.mem.torch and hasattr(e, "data_ptr"):
                import torch
                e = e.detach().to(device=self.eng.device, dtype=torch.float32).contiguous().reshape(-1)
                n = e.numel()
            else:
                e = np.ascontiguousarray(e, dtype=np.float32).reshape(-1)
                n = e.size
                e = self.mem.up(e)
                own.append(e)
            if n != spec.EMB:
                self.mem.free(*own)
                raise ValueError("set_embeddings: two rows of %d floats" % spec.EMB)
            rows.append(e)
        R = ctypes.c_int64(-1)
        try:
            hip.check(self.lib.nhans_live_set_embeddings(self.handle, int(i), self.mem.p(rows[0]), self.mem.p(rows[1]),
                                                         self.mem.stream(), ctypes.byref(R)))
        finally:
            self.mem.free(*own)
        self.conditioned[i] = True
        return int(R.value)

    def set_lookahead(self, i, L):
        """The look-ahead of slot i, L frames in 0 .. 17 (nhans_lookahead_live_set): allowed while the slot's stream has
        no samples yet -- after open or restart(i) --, kept across restarts."""
        L = spec.check_lookahead(L)
        hip.check(self.lib.nhans_lookahead_live_set(self.handle, int(i), L))
        self.lookahead[i] = L

    # ---- conditioning captured from the slot's own stream -------------------------------------
    def enable_capture(self):
        """Every slot gets its 16 kHz sample history (nhans_capture_live_enable; idempotent)."""
        hip.check(self.lib.nhans_capture_live_enable(self.handle, self.mem.stream()))

    def capture_contexts(self, pairs, normalise=True):
        """online.OnlineEnhancer.capture_contexts for the 16 kHz stage: the samples are what the incoming converter handed
        on (already divided by peak + 1e-6), resample.emitted(pushed, ended, in_rate, 16000) of them so far."""
        return online._capture_contexts(self, self.lib.nhans_capture_live_context, pairs, normalise, self.mem.stream())

    def capture_context(self, i, which, normalise=True):
        return self.capture_contexts([(i, which)], normalise)[0]

    def embeddings(self, i):
        """(a, b): slot i's current conditioning rows as two float32[512] arrays (nhans_capture_live_embeddings)."""
        return online._embeddings(self.mem, self.lib.nhans_capture_live_embeddings, self.handle, i)

    def set_wet(self, w):
        """The wet factor of the pushes that follow (non-zero needs wet=True at construction)."""
        hip.check(self.lib.nhans_live_set_wet(self.handle, float(w)))

    # ---- pushes --------------------------------------------------------------------------------
    def _endv(self, end):
        return (ctypes.c_int * self.S)(*[int(bool(e)) for e in end]) if end is not None else None

    def out_counts(self, counts, end=None):
        """nhans_live_out_counts: what a push of counts[i] samples would emit per slot."""
        out = (ctypes.c_int64 * self.S)()
        hip.check(self.lib.nhans_live_out_counts(self.handle, hip.i64_array(counts), self._endv(end), out))
        return list(out)

    def rewind(self):
        hip.check(self.lib.nhans_live_rewind(self.handle))
        self.pushed, self.ended = self._prev

    def _set_precision(self, p):
        if hasattr(self.eng, "set_precision"):
            self.eng.set_precision(p)
        else:
            self.eng.set_option("precision", {"f32": 0, "f16x3": 1}[p])

    def _push_once(self, pin, ioff, endv, pout, ooff):
        got = (ctypes.c_int64 * self.S)()
        hip.check(self.lib.nhans_live_push(self.handle, pin, hip.i64_array(ioff), endv, pout, hip.i64_array(ooff), got,
                                           self.mem.stream()))
        return list(got)

    def _push_checked(self, pin, ioff, end, pout, ooff, outc):
        """One push with nhans_live_push; a push that saturates the f16x3 path is undone and redone in f32 inside a
        raise-only calibrate bracket, as OnlineEnhancer does."""
        endv = self._endv(end)
        got = self._push_once(pin, ioff, endv, pout, ooff)
        self._prev = (list(self.pushed), list(self.ended))
        if self.eng.take_status() & hip.STATUS_SATURATED and self.eng.precision == "f16x3":
            warnings.warn("N-HANS f16x3 path: an activation left the f16 range; batch recomputed in f32 MFMA mode "
                          "and the activation exponents raised")
            hip.check(self.lib.nhans_live_rewind(self.handle))
            self.eng.set_option("calibrate", 1)
            try:
                self._set_precision("f32")
                got = self._push_once(pin, ioff, endv, pout, ooff)
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
        for i in range(self.S):
            self.pushed[i] += ioff[i + 1] - ioff[i]
            self.ended[i] = self.ended[i] or bool(end is not None and end[i])

    @staticmethod
    def _offsets(counts):
        off = [0]
        for n in counts:
            off.append(off[-1] + int(n))
        return off

    def push(self, chunks, end=None):
        """chunks: one 1-D in_dtype array per slot (may be empty); end[i]: slot i's stream ends after its chunk.  Returns
        one out_dtype array per slot: the samples that became final.  One upload of the pieces, one C call, one
        download of the results."""
        if len(chunks) != self.S:
            raise ValueError("push: one chunk per slot (%d)" % self.S)
        flat, ioff = resample._flat(chunks, self.in_dtype)
        outc = self.out_counts([ioff[i + 1] - ioff[i] for i in range(self.S)], end)
        ooff = self._offsets(outc)
        if self.mem.torch:
            import torch
            din = torch.from_numpy(flat).to(self.eng.device) if flat.size else None
            dout = torch.empty(max(ooff[-1], 1), dtype=getattr(torch, self.out_dtype.name), device=self.eng.device)
            self._push_checked(hip.ptr(din), ioff, end, hip.ptr(dout), ooff, outc)
            out = dout[:ooff[-1]].cpu().numpy()
        else:
            from . import hiprt
            din = hiprt.DevBuf.from_array(flat)
            dout = hiprt.DevBuf(self.out_dtype.itemsize * max(ooff[-1], 1))
            try:
                self._push_checked(din.ptr, ioff, end, dout.ptr, ooff, outc)
                out = dout.to_array(np.empty(ooff[-1], self.out_dtype))
            finally:
                self.mem.free(din, dout)
        return [out[ooff[i]:ooff[i + 1]] for i in range(self.S)]

    def push_device(self, samples, counts, end=None):
        """Over Engine: samples is one contiguous device tensor of in_dtype holding the slots' pieces one after the
        other, counts[i] samples for slot i.  Returns (tensor of out_dtype on the engine's device, offsets): slot i's
        results are tensor[offsets[i]:offsets[i + 1]].  No host copy of a sample either way."""
        if not self.mem.torch:
            raise TypeError("push_device needs engine.Engine (torch device memory)")
        import torch
        if len(counts) != self.S:
            raise ValueError("push_device: one count per slot (%d)" % self.S)
        ioff = self._offsets(counts)
        if samples.dtype != getattr(torch, self.in_dtype.name) or samples.device != torch.device(self.eng.device) \
                or not samples.is_contiguous() or samples.numel() < ioff[-1]:
            raise ValueError("push_device: a contiguous %s tensor on %s with at least %d samples"
                             % (self.in_dtype.name, self.eng.device, ioff[-1]))
        outc = self.out_counts(counts, end)
        ooff = self._offsets(outc)
        dout = torch.empty(max(ooff[-1], 1), dtype=getattr(torch, self.out_dtype.name), device=self.eng.device)
        self._push_checked(hip.ptr(samples), ioff, end, hip.ptr(dout), ooff, outc)
        return dout[:ooff[-1]], ooff

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nhans_live_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
