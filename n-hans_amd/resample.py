"""Sample-rate conversion on the device (include/nhans_hip.h: nhans_resample*, nhans_resampler_*, nhans_peak_normalise):
between 16 kHz and the rates capture devices deliver, for whole clips (resample) and for live streams cut into pieces
(Resampler) -- the concatenated pieces are bit for bit the conversion of the whole.  The filter is the one
scipy.signal.resample_poly designs by default, so that function is the float64 reference of this module.

Works over engine.Engine (torch device memory, the engine's current stream) and lite.LiteEngine (torch-free, hiprt
memory, the null stream).  out_count / emitted restate the contract of the header in Python so that it can be checked
without a device."""
import ctypes
from math import gcd

import numpy as np

from . import context, hip

BASE = 16000
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def supported(rate_in, rate_out):
    return (rate_in == BASE or rate_out == BASE) and rate_in in RATES and rate_out in RATES


def geometry(rate_in, rate_out):
    """-> (L, M, half, J): up and down factors, half filter length, taps per phase."""
    if not supported(rate_in, rate_out):
        raise ValueError("%d Hz -> %d Hz is not supported (one side %d Hz, the other one of %s)"
                         % (rate_in, rate_out, BASE, ", ".join(str(r) for r in RATES)))
    g = gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    if L == M == 1:
        return 1, 1, 0, 1
    half = 10 * max(L, M)
    return L, M, half, -(-(2 * half + 1) // L)


def out_count(n, rate_in, rate_out):
    """ceil(n L / M): output samples of an n-sample clip."""
    L, M, _, _ = geometry(rate_in, rate_out)
    return -(-(n * L) // M)


def emitted(n, ended, rate_in, rate_out):
    """Samples a live stream of n pushed samples has emitted in total: an output is emitted once every input it reads
    exists; an ended stream has emitted the whole clip's ceil(n L / M)."""
    L, M, half, _ = geometry(rate_in, rate_out)
    whole = -(-(n * L) // M)
    if ended:
        return whole
    return min(whole, max(0, (n * L - 1 - half) // M + 1))


def latency_ms(rate_in, rate_out):
    """Added latency of one conversion: half / (L rate_in) seconds -- 10 periods of the lower rate."""
    L, _, half, _ = geometry(rate_in, rate_out)
    return 1000.0 * half / (L * float(rate_in))


def taps(rate_in, rate_out):
    """The float64 taps the library designed (nhans_resample_taps; host only)."""
    lib = hip.load()
    n = hip.check(lib.nhans_resample_taps(int(rate_in), int(rate_out), None, 0))
    out = np.empty(n, np.float64)
    hip.check(lib.nhans_resample_taps(int(rate_in), int(rate_out), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n))
    return out


def _format(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        return hip.PCM_INT16
    if dtype == np.float32:
        return hip.PCM_FLOAT32
    raise ValueError("samples must be int16 or float32, not %s" % dtype)


def _common_dtype(arrays, dtype=None):
    if dtype is not None:
        return np.dtype(dtype)
    kinds = {np.asarray(x).dtype for x in arrays}
    return np.dtype(np.int16) if kinds == {np.dtype(np.int16)} else np.dtype(np.float32)


def resample(engine, clips, rate_in, rate_out, quantise=False):
    """clips: 1-D int16 or float32 arrays (a batch is converted in the format of all its clips: int16 if every clip is,
    else float32) -> list of float32 arrays of out_count(len) samples.  quantise: outputs on the int16 grid."""
    geometry(rate_in, rate_out)
    dtype = _common_dtype(clips)
    x, ioff = context.flat(clips, dtype)
    ooff = context.offsets(out_count(ioff[i + 1] - ioff[i], rate_in, rate_out) for i in range(len(clips)))
    mem = context.Mem(engine)
    din, dout = mem.up(x), mem.empty(ooff[-1])
    try:
        hip.check(hip.load().nhans_resample(engine.handle, mem.p(din), _format(dtype), hip.i64_array(ioff), len(clips),
                                            int(rate_in), int(rate_out), hip.RESAMPLE_QUANTISE if quantise else 0,
                                            mem.p(dout), hip.i64_array(ooff), mem.stream()))
        out = mem.down(dout, ooff[-1])
    finally:
        mem.free(din, dout)
    return [out[ooff[i]:ooff[i + 1]] for i in range(len(clips))]


def peak_normalise(engine, clips, wrap_int16=False):
    """x / (max|x| + 1e-6) per clip in float64 -> float32 on the device: apply.normalise bit for bit.  wrap_int16: the
    peak search takes |-32768| as -32768, as np.abs of an int16 array does."""
    x, off = context.flat(clips)
    mem = context.Mem(engine)
    d = mem.up(x)
    try:
        hip.check(hip.load().nhans_peak_normalise(engine.handle, mem.p(d), hip.i64_array(off), len(clips),
                                                  hip.NORMALISE_WRAP_INT16 if wrap_int16 else 0, mem.p(d), mem.stream()))
        out = mem.down(d, off[-1])
    finally:
        mem.free(d)
    return [out[off[i]:off[i + 1]] for i in range(len(clips))]


def decode_pcm(samples):
    """A wav file's samples as scipy read them, [n] or [n, channels] -> channel-major planes [channels, n] on the int16
    scale: int16 stays int16, every other format becomes float32 (uint8: (x - 128) * 256, int32: x / 65536, float:
    x * 32768 -- powers of two, the scale of the host converter).  Decoding and layout only: the signal arithmetic of the
    front end (rate conversion, rounding to the int16 grid, down-mix, normalisation) is front_end's, on the device."""
    x = np.asarray(samples)
    planes = x.reshape(len(x), -1).T
    if x.dtype == np.int16:
        return np.ascontiguousarray(planes)
    if x.dtype == np.uint8:
        return np.ascontiguousarray((planes.astype(np.float32) - np.float32(128)) * np.float32(256))
    if x.dtype == np.int32:
        return np.ascontiguousarray(planes.astype(np.float32) * np.float32(1.0 / 65536))
    if x.dtype.kind == 'f':
        return np.ascontiguousarray(planes.astype(np.float32) * np.float32(32768))
    raise ValueError("unsupported sample format %s" % x.dtype)


def front_end(engine, samples, rate, base=BASE, return_peak=False):
    """The file front end on the device: what apply.normalise(apply.read_wav_any(file)) computes on the host.  The
    channels are the clips of one ragged nhans_resample call (outputs on the int16 grid), nhans_channel_mean mixes
    them down, nhans_peak_normalise divides by the peak -- with the int16 abs wrap for a mono file, whose host array
    would have been int16 -- and only the normalised float32 signal comes back.  return_peak: -> (signal, peak), the
    peak the signal was divided by (plus 1e-6), found here from one more download of the signal before the division."""
    geometry(rate, base)
    planes = decode_pcm(samples)
    C, n = planes.shape
    no = out_count(n, rate, base)
    mem = context.Mem(engine)
    lib = hip.load()
    din, dout = mem.up(planes.reshape(-1)), mem.empty(C * no)
    try:
        hip.check(lib.nhans_resample(engine.handle, mem.p(din), _format(planes.dtype), hip.i64_array([c * n for c in range(C + 1)]),
                                     C, int(rate), int(base), hip.RESAMPLE_QUANTISE, mem.p(dout),
                                     hip.i64_array([c * no for c in range(C + 1)]), mem.stream()))
        if C > 1:
            hip.check(lib.nhans_channel_mean(engine.handle, mem.p(dout), C, no, mem.p(dout), mem.stream()))
        peak = 0.0
        if return_peak and no:
            v = np.array(mem.down(dout, no), dtype=np.float32)
            peak = float(np.max(np.where(v == -32768, v, np.abs(v)) if C == 1 else np.abs(v)))
        hip.check(lib.nhans_peak_normalise(engine.handle, mem.p(dout), hip.i64_array([0, no]), 1,
                                           hip.NORMALISE_WRAP_INT16 if C == 1 else 0, mem.p(dout), mem.stream()))
        return (mem.down(dout, no), peak) if return_peak else mem.down(dout, no)
    finally:
        mem.free(din, dout)


class Resampler:
    """nstreams live streams converted rate_in -> rate_out piece by piece (nhans_resampler_*).  dtype: what push() is
    given (int16 or float32).  peak: every output divided by (peak + 1e-6) in float64 -- online.normalise_fixed on the
    device."""

    def __init__(self, engine, nstreams, rate_in, rate_out, dtype=np.float32, quantise=False, peak=None):
        geometry(rate_in, rate_out)
        self.mem = context.Mem(engine)
        self.lib = hip.load()
        self.S = int(nstreams)
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.dtype = np.dtype(dtype)
        self.handle = None
        h = ctypes.c_void_p()
        hip.check(self.lib.nhans_resampler_open(engine.handle, self.S, self.rate_in, self.rate_out, _format(self.dtype),
                                                hip.RESAMPLE_QUANTISE if quantise else 0, ctypes.byref(h)))
        self.handle = h
        self.pushed = [0] * self.S
        self.ended = [False] * self.S
        if peak is not None:
            self.set_peak(peak)

    def set_peak(self, peak):
        hip.check(self.lib.nhans_resampler_set_peak(self.handle, float(peak)))

    def out_counts(self, counts, end=None):
        out = (ctypes.c_int64 * self.S)()
        hip.check(self.lib.nhans_resampler_out_counts(self.handle, hip.i64_array(counts), context.end_flags(end, self.S), out))
        return list(out)

    def restart(self, i):
        hip.check(self.lib.nhans_resampler_restart(self.handle, int(i)))
        self.pushed[i], self.ended[i] = 0, False

    def push(self, chunks, end=None):
        """chunks: one 1-D array per stream (may be empty); end[i]: stream i ends after its chunk.  Returns the float32
        samples of every stream that became final."""
        if len(chunks) != self.S:
            raise ValueError("push: one chunk per stream (%d)" % self.S)
        x, ioff = context.flat(chunks, self.dtype)
        counts = [ioff[i + 1] - ioff[i] for i in range(self.S)]
        outc = self.out_counts(counts, end)
        ooff = context.offsets(outc)
        din, dout = self.mem.up(x), self.mem.empty(ooff[-1])
        got = (ctypes.c_int64 * self.S)()
        try:
            hip.check(self.lib.nhans_resampler_push(self.handle, self.mem.p(din), hip.i64_array(ioff), context.end_flags(end, self.S),
                                                    self.mem.p(dout), hip.i64_array(ooff), got, self.mem.stream()))
            out = self.mem.down(dout, ooff[-1])
        finally:
            self.mem.free(din, dout)
        assert list(got) == outc, (list(got), outc)
        for i in range(self.S):
            self.pushed[i] += counts[i]
            self.ended[i] = self.ended[i] or bool(end is not None and end[i])
        return [out[ooff[i]:ooff[i + 1]] for i in range(self.S)]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nhans_resampler_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
