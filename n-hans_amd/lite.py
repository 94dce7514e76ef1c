"""LiteEngine: the whole-path entry point of the C ABI (nhans_enhance_clips) WITHOUT PyTorch -- device memory comes from
the HIP runtime through ctypes (hiprt.py), launches go to the null stream.  It is what the single-process command line
(`nhans_denoiser` / `nhans_separator` on a file or a directory, SN/apply.py:478-527, setup.py:44-50) runs on: importing
torch alone costs more wall clock than the rest of a one-file call.  Same library, same entry point, same bits as
engine.Engine.enhance (tests/test_gpu_cold_call.py); everything else -- stage-level entry points, streams, the sharded
multi-GPU path -- stays on engine.Engine.  No CPU fallback here either: no HIP device, no library -> an error."""
import ctypes

import numpy as np

from . import blobcache, context, fold, hip, hiprt, spec


class LiteEngine(context.Context):
    def __init__(self, kind, weights=None, device=0, blob=None, exponents=None, precision="f16x3"):
        """weights: checkpoint dict (folded here) -- or `blob`: an already folded blob (bytes / uint8 array, e.g. from
        blobcache) with, optionally, the activation exponents a previous context calibrated for it (the calibration
        pass of nhans_create is then skipped)."""
        self.lib = hip.load()
        if hiprt.device_count() <= device:
            raise hip.NhansError("no HIP device %d visible: the N-HANS hot path has no CPU fallback" % device)
        hiprt.check(hiprt.rt().hipSetDevice(device), "hipSetDevice")
        self.kind, self.device_index = kind, device
        if blob is None:
            blob = fold.fold_weights(weights, kind)
        arr = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        self.blob = arr                                     # (kept for blobcache.store by the caller)
        handle = ctypes.c_void_p()
        exps = None if exponents is None else (ctypes.c_int * hip.NUM_ACTIVATIONS)(*[int(e) for e in exponents])
        hip.check(self.lib.nhans_create_ex(hip.KIND_CODE[kind], arr.ctypes.data_as(ctypes.c_void_p), arr.size, device,
                                           exps, hip.NUM_ACTIVATIONS if exps is not None else 0, ctypes.byref(handle)))
        self.handle = handle
        self.set_precision(precision)

    def enhance(self, mixes, ctx_a, ctx_b, want_mixed=True, lookahead=spec.LOOKAHEAD, phase_iters=0, phase_alpha=0.0):
        """Lists of normalised float32 waveforms (mixtures trimmed) -> {"denoised_wav": [...], "mixed_wav": [...]}; the same
        saturation fallback as engine.Engine.enhance (the batch redone on the exact-f32 matrix path, exponents raised),
        the same lookahead (L frames, 0 .. 17; the redo runs with the same L) and the same phase refinement (phase_iters
        Griffin-Lim iterations of momentum phase_alpha on the denoised rows; the redo runs them too)."""
        return self._with_phase(phase_iters, phase_alpha, lambda: self._with_lookahead(
            lookahead, lambda: self._enhance(mixes, ctx_a, ctx_b, want_mixed)))

    def _enhance(self, mixes, ctx_a, ctx_b, want_mixed):
        (mf, off), (af, aoff), (bf, boff) = context.flat(mixes), context.flat(ctx_a), context.flat(ctx_b)
        for i in range(len(mixes)):
            if int(self.lib.nhans_num_frames(off[i + 1] - off[i])) == 0:
                raise ValueError("mixture clip %d has fewer than %d samples: no STFT frame" % (i, spec.WIN))
        mem = context.Mem(self)
        ins = [mem.up(x) for x in (mf, af, bf)]
        outs = []                                         # denoised, mixed round trip: those of the attempt that stands

        def launch():
            outs[:] = [hiprt.DevBuf(mf.nbytes, zero=True), hiprt.DevBuf(mf.nbytes, zero=True) if want_mixed else None]
            hip.check(self.lib.nhans_enhance_clips(
                self.handle, mem.p(ins[0]), hip.i64_array(off), len(mixes), mem.p(ins[1]), hip.i64_array(aoff),
                mem.p(ins[2]), hip.i64_array(boff), mem.p(outs[0]), mem.p(outs[1]), None, None, None, None, None))

        context.redo_saturated_in_f32(self, launch, lambda: mem.free(*outs))     # (take_status waits for the null stream)
        den = mem.down(outs[0], len(mf))
        rt = mem.down(outs[1], len(mf)) if want_mixed else None
        mem.free(*ins, *outs)
        out = {"denoised_wav": [den[off[i]:off[i + 1]] for i in range(len(mixes))], "mixed_wav": []}
        if want_mixed:
            out["mixed_wav"] = [rt[off[i]:off[i + 1]] for i in range(len(mixes))]
        return out


def cached_engine(kind, key, make_weights, device=0, use_cache=True, timing=None):
    """LiteEngine for `kind` from the blob cache entry `key` (blobcache.key_for_*), or -- no entry, a stale one,
    use_cache False -- from make_weights() folded now, the result (blob + the exponents nhans_create calibrated)
    stored for the next process.  `timing`: optional dict that receives the seconds of each step."""
    import time
    t = time.perf_counter()
    hit = blobcache.load(key) if use_cache and key else None
    if timing is not None:
        timing["cache_read_s"] = time.perf_counter() - t
        timing["cache"] = "hit" if hit else ("miss" if use_cache else "bypassed")
    if hit:
        t = time.perf_counter()
        eng = LiteEngine(kind, device=device, blob=hit[0], exponents=hit[1])
        if timing is not None:
            timing["create_s"] = time.perf_counter() - t
        if hit[1] is None:                               # (an entry written without exponents: complete it)
            blobcache.store(key, hit[0], eng.activation_exponents())
        return eng
    t = time.perf_counter()
    W = make_weights()
    t1 = time.perf_counter()
    blob = fold.fold_weights(W, kind)
    t2 = time.perf_counter()
    eng = LiteEngine(kind, device=device, blob=blob)
    if timing is not None:
        timing.update(load_weights_s=t1 - t, fold_s=t2 - t1, create_s=time.perf_counter() - t2)
    if use_cache and key:
        blobcache.store(key, blob, eng.activation_exponents())
    return eng
