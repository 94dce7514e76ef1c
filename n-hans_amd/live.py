"""Live PCM sessions (include/nhans_hip.h: nhans_live_*): pieces at the capture device's rate and format go in, pieces at
the playback device's rate and format come out, one C call per push -- rate conversion in, online enhancement, wet/dry
mix, rate conversion and PCM rounding out, with nothing on the host between the stages.  The output is bit for bit the
offline chain resample -> normalise_fixed -> trim -> enhance -> mix -> resample -> scale -> round.

LiveSession works over engine.Engine (torch device memory, the engine's current stream) and lite.LiteEngine (torch-free,
hiprt memory, the null stream).  emitted() restates the output contract of the header in Python so that it can be checked
without a device."""
import ctypes

import numpy as np

from . import context, hip, online, resample, spec


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


class LiveSession(online.Slots):
    """nslots live recordings at in_rate (in_dtype int16 or float32, every converted sample divided by peak + 1e-6) ->
    pieces at out_rate as out_dtype (int16: rounded and clipped; float32), each 16 kHz result multiplied by out_scale.
    wet=True opens the object with the mixed round trip so that set_wet(w) can blend it in:
    denoised + (mixed - denoised) * w, the reference's --compensate mix.

    Slots are the online object's (online.OnlineEnhancer): all start unconditioned; restart(i) + set_context(i, a, b)
    lets a recording join in slot i, end in a push or restart(i) lets it leave.

    lookahead: L frames, 0 .. 17, one for all slots or one per slot (set_lookahead(i, L) later, on a slot whose stream
    has no samples yet): the 16 kHz stage then computes the offline output of that L, Engine.enhance(..., lookahead=L).

    capture_contexts: the samples are what the incoming converter handed on (already divided by peak + 1e-6),
    resample.emitted(pushed, ended, in_rate, 16000) of them so far."""

    C = dict(restart="nhans_live_restart", rewind="nhans_live_rewind", out_counts="nhans_live_out_counts",
             set_context="nhans_live_set_context", set_embeddings="nhans_live_set_embeddings",
             set_lookahead="nhans_lookahead_live_set", capture_enable="nhans_capture_live_enable",
             capture_context="nhans_capture_live_context", capture_embeddings="nhans_capture_live_embeddings",
             close="nhans_live_close")

    def __init__(self, engine, nslots, in_rate, out_rate, peak, in_dtype=np.int16, out_dtype=np.int16, out_scale=None,
                 wet=False, lookahead=online.LOOKAHEAD):
        emitted(0, False, in_rate, out_rate)
        self._begin(engine, nslots, False)
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.in_dtype, self.out_dtype = np.dtype(in_dtype), np.dtype(out_dtype)
        self.peak = float(peak)
        self.out_scale = default_out_scale(peak, out_dtype) if out_scale is None else float(out_scale)
        self.has_wet = bool(wet)
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_live_open_slots(engine.handle, self.S, self.in_rate, resample._format(self.in_dtype),
                                                 self.peak, self.out_rate, resample._format(self.out_dtype), self.out_scale,
                                                 hip.LIVE_WET if self.has_wet else 0, self.mem.stream(), ctypes.byref(h)))
        self.handle = h
        self._lookaheads(lookahead)

    def set_wet(self, w):
        """The wet factor of the pushes that follow (non-zero needs wet=True at construction)."""
        hip.check(self.lib.nhans_live_set_wet(self.handle, float(w)))

    # ---- pushes --------------------------------------------------------------------------------
    def _push(self, pin, ioff, end, dout, ooff, outc):
        """One nhans_live_push of the pieces at device pointer pin into the device buffer dout."""
        def push():
            got = (ctypes.c_int64 * self.S)()
            hip.check(self.lib.nhans_live_push(self.handle, pin, hip.i64_array(ioff), context.end_flags(end, self.S),
                                               self.mem.p(dout), hip.i64_array(ooff), got, self.mem.stream()))
            return list(got)

        self._push_checked(push, [ioff[i + 1] - ioff[i] for i in range(self.S)], end, outc)

    def push(self, chunks, end=None):
        """chunks: one 1-D in_dtype array per slot (may be empty); end[i]: slot i's stream ends after its chunk.  Returns
        one out_dtype array per slot: the samples that became final.  One upload of the pieces, one C call, one
        download of the results."""
        if len(chunks) != self.S:
            raise ValueError("push: one chunk per slot (%d)" % self.S)
        x, ioff = context.flat(chunks, self.in_dtype)
        outc = self.out_counts([ioff[i + 1] - ioff[i] for i in range(self.S)], end)
        ooff = context.offsets(outc)
        din, dout = self.mem.up(x), self.mem.empty(ooff[-1], self.out_dtype)
        try:
            self._push(self.mem.p(din), ioff, end, dout, ooff, outc)
            out = self.mem.down(dout, ooff[-1], self.out_dtype)
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
        ioff = context.offsets(counts)
        if samples.dtype != getattr(torch, self.in_dtype.name) or samples.device != torch.device(self.eng.device) \
                or not samples.is_contiguous() or samples.numel() < ioff[-1]:
            raise ValueError("push_device: a contiguous %s tensor on %s with at least %d samples"
                             % (self.in_dtype.name, self.eng.device, ioff[-1]))
        outc = self.out_counts(counts, end)
        ooff = context.offsets(outc)
        dout = self.mem.empty(ooff[-1], self.out_dtype)
        self._push(hip.ptr(samples), ioff, end, dout, ooff, outc)
        return dout[:ooff[-1]], ooff
