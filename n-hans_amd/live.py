"""Live PCM sessions (include/nhans_hip.h: nhans_live_*): pieces at the capture device's rate and format go in, pieces at
the playback device's rate and format come out, one C call per push -- rate conversion in, online enhancement, wet/dry
mix, rate conversion and PCM rounding out, with nothing on the host between the stages.  The output is bit for bit the
offline chain resample -> normalise_fixed -> trim -> enhance -> mix -> resample -> scale -> round.

LiveSession works over engine.Engine (torch device memory, the engine's current stream) and lite.LiteEngine (torch-free,
hiprt memory, the null stream).  emitted() restates the output contract of the header in Python so that it can be checked
without a device."""
import ctypes
import math

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


def level_hops(emitted, ended):
    """nhans_level_hops restated: final hops of a stream that has emitted `emitted` 16 kHz samples."""
    if emitted < 0:
        raise ValueError("level_hops: negative sample count")
    return -(-emitted // spec.HOP) if ended else emitted // spec.HOP


def _dbfs(power, samples):
    """10 log10 of the mean square of `samples` samples whose squares sum to `power` (-inf for silence)."""
    return 10.0 * math.log10(power / samples) if power > 0 and samples > 0 else -math.inf


def level_gains(engine, den, mix, window_hops=200, wmax=1.0, sums=False):
    """The per-hop automatic wet factors of whole 16 kHz clips (nhans_level_gains: the kernel of a live session's meter
    over ended streams that start at hop 0): den / mix one float32 array or a list of them, window_hops 0 .. 256 (0:
    cumulative, the reference's --ac figure to date), wmax the clamp.  Returns one float32 array of ceil(n / 160) gains
    per clip (a single array for a single array); with sums=True also the eight doubles nhans_level_live_read defines,
    per clip."""
    single = isinstance(den, np.ndarray) and den.ndim == 1
    dens, mixes = ([den], [mix]) if single else (list(den), list(mix))
    if len(dens) != len(mixes) or any(len(d) != len(m) for d, m in zip(dens, mixes)):
        raise ValueError("level_gains: den and mix are the same clips, sample for sample")
    mem = context.Mem(engine)
    d, off = context.flat(dens)
    m, _ = context.flat(mixes)
    hoff = context.offsets(level_hops(len(x), True) for x in dens)
    dd, dm = mem.up(d), mem.up(m)
    dw, ds = mem.empty(hoff[-1]), mem.empty(8 * len(dens), np.float64)
    try:
        hip.check(hip.load().nhans_level_gains(engine.handle, mem.p(dd), mem.p(dm), hip.i64_array(off), len(dens),
                                               int(window_hops), float(wmax), mem.p(dw), mem.p(ds), mem.stream()))
        w = np.array(mem.down(dw, hoff[-1]), dtype=np.float32)
        s = np.array(mem.down(ds, 8 * len(dens), np.float64), dtype=np.float64).reshape(len(dens), 8)
    finally:
        mem.free(dd, dm, dw, ds)
    gains = [w[hoff[i]:hoff[i + 1]].copy() for i in range(len(dens))]
    if single:
        return (gains[0], s[0]) if sums else gains[0]
    return (gains, s) if sums else gains


def fullband_hold(rate):
    """nhans_fullband_hold_samples: H(rate), the input samples a full-band slot keeps at most while their output is
    still to come."""
    return hip.check(hip.load().nhans_fullband_hold_samples(int(rate)))


def fullband_mix(engine, x, den, mix, rate, in_denom, wet=0.0, gain=1.0, out_dtype=np.int16, out_scale=1.0, wet_hops=None):
    """The whole-clip twin of a full-band live session (nhans_fullband_mix: the kernels of its ended streams).  x: the
    recording at `rate` (int16 or float32; one array or a list), den / mix its final 16 kHz denoised and mixed-round-trip
    samples, in_denom the divisor the 16 kHz path normalised by (peak + 1e-6).  Returns
    y = R(c - gain * mix) + gain * float32(x / in_denom) per clip as out_dtype through the outgoing sink's arithmetic
    (times out_scale, rounded and clipped for int16), c = den + (mix - den) * wet -- or, with wet_hops, one factor per
    160-sample hop of each clip (level_gains' arrays) -- and R the conversion 16 kHz -> rate: resample.out_count(len(den),
    16000, rate) samples, the first aligned with x[0]."""
    single = isinstance(den, np.ndarray) and den.ndim == 1
    xs, dens, mixes = ([x], [den], [mix]) if single else (list(x), list(den), list(mix))
    hops = None if wet_hops is None else ([wet_hops] if single else list(wet_hops))
    if not (len(xs) == len(dens) == len(mixes)) or any(len(d) != len(m) for d, m in zip(dens, mixes)):
        raise ValueError("fullband_mix: x, den and mix are the same clips, den and mix sample for sample")
    if hops is not None and [len(h) for h in hops] != [level_hops(len(d), True) for d in dens]:
        raise ValueError("fullband_mix: wet_hops holds one factor per hop of 160 samples of each clip")
    x_dtype = np.dtype(np.int16) if all(np.asarray(v).dtype == np.int16 for v in xs) else np.dtype(np.float32)
    out_dtype = np.dtype(out_dtype)
    lib, mem = hip.load(), context.Mem(engine)
    xf, xoff = context.flat(xs, x_dtype)
    d, off = context.flat(dens)
    m, _ = context.flat(mixes)
    ooff = context.offsets(hip.check(lib.nhans_resample_out_count(len(v), spec.FS, int(rate))) for v in dens)
    bufs = [mem.up(xf), mem.up(d), mem.up(m), mem.empty(ooff[-1], out_dtype)]
    if hops is not None:
        bufs.append(mem.up(context.flat(hops)[0]))
    try:
        hip.check(lib.nhans_fullband_mix(engine.handle, mem.p(bufs[0]), resample._format(x_dtype), hip.i64_array(xoff), mem.p(bufs[1]),
                                         mem.p(bufs[2]), hip.i64_array(off), len(dens), int(rate), float(in_denom), float(wet),
                                         mem.p(bufs[4]) if hops is not None else None, float(gain), float(out_scale),
                                         resample._format(out_dtype), mem.p(bufs[3]), hip.i64_array(ooff), mem.stream()))
        y = np.array(mem.down(bufs[3], ooff[-1], out_dtype), dtype=out_dtype)
    finally:
        mem.free(*bufs)
    out = [y[ooff[i]:ooff[i + 1]].copy() for i in range(len(dens))]
    return out[0] if single else out


def downmix(frames):
    """The sample a downmix session forms from each interleaved frame (include/nhans_hip.h, NHANS_INTERLEAVED_DOWNMIX):
    frames [n, C] (or [n]: one channel) -> float32 [n], float32((sum_c float64(frames[k, c])) / float64(C)) with the sum
    starting at 0.0 and adding c in ascending order -- an explicit loop: the order of numpy's own reductions is numpy's
    choice.  One channel comes back as it is."""
    x = np.asarray(frames)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("downmix: frames [n, C] with C >= 1")
    acc = np.zeros(x.shape[0], dtype=np.float64)
    for c in range(x.shape[1]):
        acc = acc + x[:, c].astype(np.float64)
    return (acc / np.float64(x.shape[1])).astype(np.float32)


CHANNEL_MODES = {"downmix": hip.INTERLEAVED_DOWNMIX, "split": hip.INTERLEAVED_SPLIT}


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
    resample.emitted(pushed, ended, in_rate, 16000) of them so far.

    channels / out_channels (1 .. 8; out_channels None: as channels) other than 1: nslots counts STREAMS of interleaved
    frames (nhans_interleaved_*) -- push takes one [frames, channels] array per stream and returns [frames, out_channels]
    arrays.  channel_mode "downmix": one slot per stream, fed downmix(frames), its output copied to every output
    channel.  "split" (channels == out_channels): one slot per channel, slots_of(stream), each enhanced on its own; the
    per-slot calls (set_context, restart, set_lookahead, capture_context, levels, ...) take those slot indices, and the
    slots of a stream have to be restarted and given their look-ahead together.  Gains are per slot: set_auto_wet may
    move the channels of a stream differently."""

    C = dict(restart="nhans_live_restart", rewind="nhans_live_rewind", out_counts="nhans_live_out_counts",
             set_context="nhans_live_set_context", set_embeddings="nhans_live_set_embeddings",
             set_lookahead="nhans_lookahead_live_set", capture_enable="nhans_capture_live_enable",
             capture_context="nhans_capture_live_context", capture_embeddings="nhans_capture_live_embeddings",
             fbank_attach="nhans_fbank_live_attach", fbank_read="nhans_fbank_live_read", close="nhans_live_close")

    def __init__(self, engine, nslots, in_rate, out_rate, peak, in_dtype=np.int16, out_dtype=np.int16, out_scale=None,
                 wet=False, lookahead=online.LOOKAHEAD, channels=1, out_channels=None, channel_mode="downmix"):
        emitted(0, False, in_rate, out_rate)
        self.channels = int(channels)
        self.out_channels = self.channels if out_channels is None else int(out_channels)
        self.interleaved = (self.channels, self.out_channels) != (1, 1)
        if channel_mode not in CHANNEL_MODES:
            raise ValueError("channel_mode: 'downmix' or 'split' (got %r)" % (channel_mode,))
        self.split = self.interleaved and channel_mode == "split"
        self.nstreams = int(nslots)
        self._begin(engine, self.nstreams * (self.channels if self.split else 1), False)
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.in_dtype, self.out_dtype = np.dtype(in_dtype), np.dtype(out_dtype)
        self.peak = float(peak)
        self.out_scale = default_out_scale(peak, out_dtype) if out_scale is None else float(out_scale)
        self.has_wet = bool(wet)
        self._level_window = 0          # (the meter's window: cumulative until set_auto_wet names one)
        h = ctypes.c_void_p()
        tail = (self.in_rate, resample._format(self.in_dtype), self.peak, self.out_rate, resample._format(self.out_dtype),
                self.out_scale, hip.LIVE_WET if self.has_wet else 0, self.mem.stream(), ctypes.byref(h))
        if self.interleaved:
            hip.check(self.lib.nhans_interleaved_live_open(engine.handle, self.nstreams, self.channels, self.out_channels,
                                                           CHANNEL_MODES[channel_mode], *tail))
        else:
            hip.check(self.lib.nhans_live_open_slots(engine.handle, self.S, *tail))
        self.handle = h
        self._lookaheads(lookahead)

    def slots_of(self, stream):
        """The slot indices of `stream` for the per-slot calls: one slot, or in split mode one per channel, in channel
        order."""
        if not 0 <= int(stream) < self.nstreams:
            raise ValueError("slots_of: stream %r out of range (0 ... %d)" % (stream, self.nstreams - 1))
        k = self.S // self.nstreams
        return list(range(int(stream) * k, int(stream) * k + k))

    def out_counts(self, counts, end=None):
        """What a push of counts[i] samples would emit per slot -- with interleaved frames: of counts[g] frames per
        stream, in frames."""
        if not self.interleaved:
            return super().out_counts(counts, end)
        if len(counts) != self.nstreams:
            raise ValueError("out_counts: one count per stream (%d)" % self.nstreams)
        out = (ctypes.c_int64 * self.nstreams)()
        hip.check(self.lib.nhans_interleaved_live_out_counts(self.handle, hip.i64_array(counts),
                                                             context.end_flags(end, self.nstreams), out))
        return list(out)

    def set_wet(self, w):
        """The wet factor of the pushes that follow (non-zero needs wet=True at construction)."""
        hip.check(self.lib.nhans_live_set_wet(self.handle, float(w)))

    # ---- full-band output (include/nhans_hip.h: nhans_fullband_*) -------------------------------
    def enable_fullband(self):
        """The band above 8 kHz, which the 16 kHz path cannot carry, comes from the input itself: every slot keeps the
        input samples that have no output yet, and each output sample gets gain * (input - its own trip through 16 kHz)
        added, aligned sample for sample (needs in_rate == out_rate > 16000, wet=True and slots that have taken no sample
        yet; idempotent).  The gain starts at 1.0 for every slot; one small launch more per push.  With set_wet(1.0) and
        gain 1.0 an int16 session on its default scale returns its input.  In "downmix" mode the high band is that of the
        downmix, on every output channel; a high band per channel needs "split"."""
        hip.check(self.lib.nhans_fullband_live_enable(self.handle, self.mem.stream()))

    def set_highband(self, g, slot=None):
        """The high-band gain, 0 .. 4, of `slot` (None: of every slot) for the pushes that follow; 0 is the output of a
        session without the feature."""
        hip.check(self.lib.nhans_fullband_live_set_gain(self.handle, -1 if slot is None else int(slot), float(g)))

    # ---- level meter and automatic compensation (include/nhans_hip.h: nhans_level_*) -----------
    def enable_levels(self):
        """Every slot gets its level state (needs wet=True; idempotent): pushes from now on also meter the hops they
        make final, one small launch more per push."""
        hip.check(self.lib.nhans_level_live_enable(self.handle, self.mem.stream()))

    def set_auto_wet(self, window_hops=200, wmax=1.0):
        """The reference's --ac, live: the hops later pushes make final are mixed with
        w = clip((Sd / Sr) / 20, 0, wmax), Sd and Sr the denoised and the removed power of the last window_hops hops
        (10 ms each, 1 .. 256; 0: of the whole stream so far).  The factor is constant over a hop and steps between
        hops: a short window follows the signal and steps more.  None switches back to the factor of set_wet, which
        stays stored (and can be set) meanwhile.  Needs enable_levels()."""
        if window_hops is None:
            hip.check(self.lib.nhans_level_live_auto(self.handle, -1, 0.0))
        else:
            hip.check(self.lib.nhans_level_live_auto(self.handle, int(window_hops), float(wmax)))
            self._level_window = int(window_hops)

    def levels(self, slot):
        """The meter of `slot` after its last final hop (one small copy, one stream sync): the window sums sd / sr / sm
        (denoised, removed, mixed), hops, the law's gain w of that hop, snr_est = sd / sr, and the three levels in dBFS
        over the window's samples -- derived here from the sums, taking every hop as 160 samples.  NhansError with
        .code == hip.ESHORT before the slot's first hop."""
        out = (ctypes.c_double * 8)()
        hip.check(self.lib.nhans_level_live_read(self.handle, int(slot), out, self.mem.stream()))
        sd, sr, sm, hops, w, snr = (float(v) for v in out[:6])
        n = spec.HOP * (min(self._level_window, int(hops)) if self._level_window else int(hops))
        return dict(sd=sd, sr=sr, sm=sm, hops=int(hops), w=w, snr_est=snr, denoised_dbfs=_dbfs(sd, n),
                    removed_dbfs=_dbfs(sr, n), mixed_dbfs=_dbfs(sm, n))

    def last_gains(self, slot):
        """The gains of the hops the last push made final for `slot` (float32, hop order; empty after a rewind)."""
        n = hip.check(self.lib.nhans_level_live_gains(self.handle, int(slot), None, 0, self.mem.stream()))
        out = (ctypes.c_float * max(n, 1))()
        if n:
            hip.check(self.lib.nhans_level_live_gains(self.handle, int(slot), out, n, self.mem.stream()))
        return np.array(out[:n], dtype=np.float32)

    # ---- pushes --------------------------------------------------------------------------------
    def _push(self, pin, ioff, end, dout, ooff, outc):
        """One nhans_live_push of the pieces at device pointer pin into the device buffer dout -- with interleaved
        frames, one nhans_interleaved_live_push: offsets and counts per stream, in frames."""
        n = self.nstreams
        entry = self.lib.nhans_interleaved_live_push if self.interleaved else self.lib.nhans_live_push

        def push():
            got = (ctypes.c_int64 * n)()
            hip.check(entry(self.handle, pin, hip.i64_array(ioff), context.end_flags(end, n), self.mem.p(dout),
                            hip.i64_array(ooff), got, self.mem.stream()))
            return list(got)

        # (the host's view is per slot: the slots of a split stream each take the stream's frames and its end)
        k = self.S // n
        counts = [ioff[i // k + 1] - ioff[i // k] for i in range(self.S)]
        self._push_checked(push, counts, end if end is None or k == 1 else [end[i // k] for i in range(self.S)], outc)

    def _push_frames(self, chunks, end):
        if len(chunks) != self.nstreams:
            raise ValueError("push: one [frames, %d] array per stream (%d)" % (self.channels, self.nstreams))
        arrs = []
        for c in chunks:
            a = np.asarray(c, dtype=self.in_dtype)
            if a.ndim == 1 and (self.channels == 1 or a.size == 0):
                a = a.reshape(-1, self.channels)
            if a.ndim != 2 or a.shape[1] != self.channels:
                raise ValueError("push: one [frames, %d] array per stream" % self.channels)
            arrs.append(a)
        ioff = context.offsets(len(a) for a in arrs)
        x = np.ascontiguousarray(np.concatenate(arrs), dtype=self.in_dtype).reshape(-1)
        outc = self.out_counts([len(a) for a in arrs], end)
        ooff = context.offsets(outc)
        co = self.out_channels
        din, dout = self.mem.up(x), self.mem.empty(ooff[-1] * co, self.out_dtype)
        try:
            self._push(self.mem.p(din), ioff, end, dout, ooff, outc)
            out = self.mem.down(dout, ooff[-1] * co, self.out_dtype).reshape(-1, co)
        finally:
            self.mem.free(din, dout)
        return [out[ooff[g]:ooff[g + 1]] for g in range(self.nstreams)]

    def push(self, chunks, end=None):
        """chunks: one 1-D in_dtype array per slot (may be empty); end[i]: slot i's stream ends after its chunk.  Returns
        one out_dtype array per slot: the samples that became final.  One upload of the pieces, one C call, one
        download of the results.  With interleaved frames: one [frames, channels] array per stream in, one
        [frames, out_channels] array per stream out."""
        if self.interleaved:
            return self._push_frames(chunks, end)
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
        results are tensor[offsets[i]:offsets[i + 1]].  No host copy of a sample either way.
        With interleaved frames: samples is the flat interleaved tensor, counts[g] FRAMES of `channels` elements for
        stream g, and stream g's results are the frames tensor[offsets[g] * out_channels:offsets[g + 1] * out_channels]."""
        if not self.mem.torch:
            raise TypeError("push_device needs engine.Engine (torch device memory)")
        import torch
        if len(counts) != self.nstreams:
            raise ValueError("push_device: one count per %s (%d)" % ("stream" if self.interleaved else "slot", self.nstreams))
        ioff = context.offsets(counts)
        if samples.dtype != getattr(torch, self.in_dtype.name) or samples.device != torch.device(self.eng.device) \
                or not samples.is_contiguous() or samples.numel() < ioff[-1] * self.channels:
            raise ValueError("push_device: a contiguous %s tensor on %s with at least %d samples"
                             % (self.in_dtype.name, self.eng.device, ioff[-1] * self.channels))
        outc = self.out_counts(counts, end)
        ooff = context.offsets(outc)
        dout = self.mem.empty(ooff[-1] * self.out_channels, self.out_dtype)
        self._push(hip.ptr(samples), ioff, end, dout, ooff, outc)
        return dout[:ooff[-1] * self.out_channels], ooff
