"""Device-side engine: owns one libnhans_hip context and moves ragged clip batches through it.
PyTorch is used only for device memory and streams; all arithmetic runs in the HIP library."""
import ctypes
import os

import torch

from . import context, fold, hip, score as score_mod, spec, weights as weights_mod


def _pair_check(who, est_t, est_off, tgt_t, tgt_off):
    """What the *_device methods (`who`) on estimate / target pairs ask of their arguments -> the number of pairs."""
    n = len(est_off) - 1
    if len(tgt_off) - 1 != n:
        raise ValueError("%s: one target per estimate" % who)
    for t in (est_t, tgt_t):
        if t.dtype != torch.float32 or t.dim() != 1:
            raise ValueError("%s: flat float32 tensors" % who)
    return n


class Engine(context.Context):
    """kind: 'denoiser' | 'separator'.  weights: checkpoint dict (name -> float32 array) or None for
    the seeded synthetic weights.  Conditioning order everywhere is (a, b) = resnet_block argument
    order: denoiser (pos, neg); separator (noise = --neg, clean = --pos)."""

    torch_memory = True

    def __init__(self, kind=spec.DENOISER, weights=None, device=0, seed=7, frames_per_chunk=None,
                 precision=None):
        if not torch.cuda.is_available():
            raise hip.NhansError("no HIP device visible: the N-HANS hot path has no CPU fallback")
        self.lib = hip.load()
        self.kind = kind
        self.device = torch.device("cuda", device)
        if weights is None:
            weights = weights_mod.synthetic_weights(kind, seed)
        blob = fold.fold_weights(weights, kind)
        handle = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(blob, len(blob))
        hip.check(self.lib.nhans_create(hip.KIND_CODE[kind], buf, len(blob), device, ctypes.byref(handle)))
        self.handle = handle
        if frames_per_chunk:
            self.set_option("frames_per_chunk", frames_per_chunk)
        self.set_precision(precision)
        if "NHANS_CONV_VARIANT" in os.environ:
            self.set_option("conv_variant", int(os.environ["NHANS_CONV_VARIANT"]))

    def set_precision(self, precision):
        """context.Context.set_precision; None: $NHANS_PRECISION, else 'f16x3'."""
        if precision is None:
            precision = os.environ.get("NHANS_PRECISION", "f16x3")
        super().set_precision(precision)

    def calibrate(self, mixes, ctx_a, ctx_b, raise_only=False):
        """Sets the activation exponents from the caller's own clips (nhans_create has calibrated on a built-in
        signal): one f32-mode pass with every tensor's maximum recorded."""
        before = self.precision
        self.set_option("calibrate", 1)
        try:
            self.set_precision("f32")
            mix_t, mix_off = self._dev(mixes)
            ca_t, ca_off = self._dev(ctx_a)
            cb_t, cb_off = self._dev(ctx_b)
            self.enhance_device(mix_t, mix_off, ca_t, ca_off, cb_t, cb_off)
        except BaseException:
            # the pass failed: close the bracket FIRST (3 = keep the exponents, learn nothing) -- an open bracket keeps
            # recording maxima on every later call --, then put the precision back; neither may mask the original error
            try:
                self.set_option("calibrate", 3)
            finally:
                self.set_precision(before)
            raise
        try:
            self.set_option("calibrate", 2 if raise_only else 0)
        finally:
            self.set_precision(before)
        return self.activation_exponents()

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, arrays):
        """list of 1-D float32 numpy arrays -> (concatenated device tensor, offsets)."""
        flat, off = context.flat(arrays)
        return torch.from_numpy(flat).to(self.device), off

    # ---- stage-level entry points (used by the parity tests) --------------------------------
    def stft_features(self, wav_t, sample_off, max_frames=0, want_phase=True):
        n = len(sample_off) - 1
        tot = 0
        for i in range(n):
            t = int(self.lib.nhans_num_frames(sample_off[i + 1] - sample_off[i]))
            tot += min(t, max_frames) if max_frames > 0 else t
        lm = torch.empty((tot, spec.BINS), dtype=torch.float32, device=self.device)
        ph = torch.empty_like(lm) if want_phase else None
        hip.check(self.lib.nhans_stft_features(self.handle, hip.ptr(wav_t), hip.i64_array(sample_off), n,
                                               max_frames, hip.ptr(lm), hip.ptr(ph), self._stream()))
        return lm, ph

    def embed(self, ctx_lm):
        n = ctx_lm.shape[0]
        out = torch.empty((n, spec.EMB), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_embed(self.handle, hip.ptr(ctx_lm.contiguous()), n, hip.ptr(out), self._stream()))
        return out

    def mask_net(self, logmag, frame_off, emb_a, emb_b, want_logits=True):
        den = torch.empty_like(logmag)
        lg = torch.empty_like(logmag) if want_logits else None
        hip.check(self.lib.nhans_mask_net(self.handle, hip.ptr(logmag), hip.i64_array(frame_off), len(frame_off) - 1,
                                          hip.ptr(emb_a.contiguous()), hip.ptr(emb_b.contiguous()), hip.ptr(lg),
                                          hip.ptr(den), self._stream()))
        return lg, den

    def block_output(self, logmag, frame_off, emb_a, emb_b, frame0, nframes, block):
        g = (spec.main_geometry() + [dict(hout=1, wout=26, cout=512)])[block]
        out = torch.empty((nframes, g["hout"], g["wout"], g["cout"]), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_debug_block_output(
            self.handle, hip.ptr(logmag), hip.i64_array(frame_off), len(frame_off) - 1, hip.ptr(emb_a.contiguous()),
            hip.ptr(emb_b.contiguous()), frame0, nframes, block, hip.ptr(out), self._stream()))
        return out

    def activation(self, index, logmag, frame_off, emb_a, emb_b, frame0, nframes):
        """Stored tensor `index` (8 .. 24, hip.NUM_ACTIVATIONS numbering) of the stack for frames [frame0, frame0 + nframes),
        f32 NHWC, written by the production launches in passes of frames_per_chunk (nhans_debug_activation)."""
        g = spec.activation_geometry()[index] if 8 <= index < hip.NUM_ACTIVATIONS else dict(hout=1, wout=1, cout=1)
        out = torch.empty((max(nframes, 0), g["hout"], g["wout"], g["cout"]), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_debug_activation(
            self.handle, hip.ptr(logmag), hip.i64_array(frame_off), len(frame_off) - 1, hip.ptr(emb_a.contiguous()),
            hip.ptr(emb_b.contiguous()), frame0, nframes, index, hip.ptr(out), self._stream()))
        return out

    def tower_activation(self, index, ctx_lm):
        """Stored tensor `index` (0 .. 7) of the embedding tower for the context images ctx_lm [n,200,201], f32 NHWC
        (nhans_debug_tower_activation: nhans_embed's launches)."""
        n = ctx_lm.shape[0]
        g = spec.activation_geometry()[index] if 0 <= index < 8 else dict(hout=1, wout=1, cout=1)
        out = torch.empty((n, g["hout"], g["wout"], g["cout"]), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_debug_tower_activation(self.handle, hip.ptr(ctx_lm.contiguous()), n, index, hip.ptr(out),
                                                        self._stream()))
        return out

    def istft(self, logmag, phase, frame_off):
        lens = [(frame_off[i + 1] - frame_off[i] - 1) * spec.HOP + spec.WIN if frame_off[i + 1] > frame_off[i] else 0
                for i in range(len(frame_off) - 1)]
        ooff = context.offsets(lens)
        out = torch.zeros(ooff[-1], dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_istft(self.handle, hip.ptr(logmag), hip.ptr(phase), hip.i64_array(frame_off),
                                       len(frame_off) - 1, hip.i64_array(ooff), hip.ptr(out), self._stream()))
        return out, ooff

    # ---- phase refinement (include/nhans_hip.h: nhans_phase_*) ----------------------------------------
    def _phase_rows_check(self, who, frame_off, real, cplx=()):
        for t in real:
            if t.dim() != 2 or t.shape != (int(frame_off[-1]), spec.BINS) or t.dtype != torch.float32:
                raise ValueError("%s: float32 [%d, %d] rows" % (who, frame_off[-1], spec.BINS))
        for t in cplx:
            if t.shape != (int(frame_off[-1]), spec.BINS) or t.dtype != torch.complex64:
                raise ValueError("%s: a complex64 [%d, %d] state" % (who, frame_off[-1], spec.BINS))

    def phase_project_rows(self, logmag, t, frame_off, inc=False):
        """One projection d = P(logmag, t) of device tensors: logmag float32 [F, 201], t complex64 [F, 201], clip i = rows
        frame_off[i]:frame_off[i + 1] -> d complex64 [F, 201]; inc=True: -> (d, float64 [n]: each clip's inconsistency)."""
        self._phase_rows_check("phase_project_rows", frame_off, (logmag,), (t,))
        n = len(frame_off) - 1
        d = torch.empty_like(t)
        ic = torch.empty(max(n, 1), dtype=torch.float64, device=self.device) if inc else None
        hip.check(self.lib.nhans_phase_project(self.handle, hip.ptr(logmag.contiguous()), hip.ptr(torch.view_as_real(t.contiguous())),
                                               hip.i64_array(frame_off), n, hip.ptr(torch.view_as_real(d)), hip.ptr(ic), self._stream()))
        return (d, ic[:n]) if inc else d

    def phase_refine_rows(self, logmag, phase, frame_off, iters, alpha=0.0, inc=False):
        """iters Griffin-Lim iterations of momentum alpha on device tensors: logmag and phase float32 [F, 201], clip i = rows
        frame_off[i]:frame_off[i + 1] -> the refined phases, float32 [F, 201] (iters = 0: the input's bits); inc=True: ->
        (that, float64 [n, iters]: inc[n] of every clip).  The waveform is istft(logmag, refined phases, frame_off)."""
        self._phase_rows_check("phase_refine_rows", frame_off, (logmag, phase))
        n, N = len(frame_off) - 1, int(iters)
        out = torch.empty_like(phase)
        ic = torch.empty((max(n, 1), max(N, 1)), dtype=torch.float64, device=self.device) if inc else None
        hip.check(self.lib.nhans_phase_refine(self.handle, hip.ptr(logmag.contiguous()), hip.ptr(phase.contiguous()),
                                              hip.i64_array(frame_off), n, N, float(alpha), hip.ptr(out), hip.ptr(ic), self._stream()))
        return (out, ic[:n, :N].contiguous() if N else ic[:n, :0]) if inc else out

    # ---- mask-driven MVDR beamforming (include/nhans_hip.h: nhans_mvdr_*) ------------------------------
    def mvdr_device(self, planes_t, sample_off, channels, mask_t, ref=0, loading=1e-6, loggain=False, gain_t=None):
        """The beamformer on tensors already in HBM.  planes_t: flat float32, clip i = `channels` planes of n_i = sample_off[i
        + 1] - sample_off[i] samples from element channels * sample_off[i] on; mask_t: float32 [F, 201] rows at the clips'
        frame offsets (loggain=True: a log-gain, mask_net's logits); gain_t (optional): float32 [F, 201] log-gain added to
        the output -> dict of device tensors: "logmag" and "phase" float32 [F, 201], "w" complex128 [n, 201, channels],
        "records" float64 [n, hip.MVDR_FIELDS] (mvdr.FIELDS names the columns), and "frame_off"."""
        n, C = len(sample_off) - 1, int(channels)
        foff = context.offsets(int(self.lib.nhans_num_frames(sample_off[i + 1] - sample_off[i])) for i in range(n))
        F = foff[-1]
        if planes_t.dtype != torch.float32 or planes_t.dim() != 1 or planes_t.numel() != C * sample_off[-1]:
            raise ValueError("mvdr_device: a flat float32 tensor of %d planes per clip" % C)
        for t in (mask_t, gain_t):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (F, spec.BINS)):
                raise ValueError("mvdr_device: float32 [%d, %d] rows" % (F, spec.BINS))
        lm = torch.empty((max(F, 1), spec.BINS), dtype=torch.float32, device=self.device)
        ph = torch.empty_like(lm)
        w = torch.empty((max(n, 1), spec.BINS, max(C, 1)), dtype=torch.complex128, device=self.device)
        rec = torch.empty((max(n, 1), hip.MVDR_FIELDS), dtype=torch.float64, device=self.device)
        hip.check(self.lib.nhans_mvdr(self.handle, hip.ptr(planes_t.contiguous()), hip.i64_array(sample_off), n, C, hip.ptr(mask_t.contiguous()),
                                      int(ref), float(loading), hip.MVDR_LOGGAIN if loggain else 0,
                                      hip.ptr(gain_t.contiguous()) if gain_t is not None else None, hip.ptr(lm), hip.ptr(ph),
                                      hip.ptr(torch.view_as_real(w)), hip.ptr(rec), self._stream()))
        return {"logmag": lm[:F], "phase": ph[:F], "w": w[:n], "records": rec[:n], "frame_off": foff}

    def fbank_rows(self, rows_t, fb):
        """fb (fbank.Filterbank) applied to a device tensor of [n, 201] float32 log-magnitude rows -- mask_net's denoised
        rows, or stft_features' logmag for the unprocessed signal -- -> device tensor [n, fb.n_mels]."""
        if rows_t.dim() != 2 or rows_t.shape[1] != spec.BINS or rows_t.dtype != torch.float32:
            raise ValueError("fbank_rows: a float32 [n, %d] tensor" % spec.BINS)
        rows_t = rows_t.contiguous()
        out = torch.empty((rows_t.shape[0], fb.n_mels), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_fbank_rows(fb.handle(self), hip.ptr(rows_t), rows_t.shape[0], hip.ptr(out), self._stream()))
        return out

    # ---- scoring against a clean target (include/nhans_hip.h: nhans_score_*) ----------------------
    def score_device(self, est_t, est_off, tgt_t, tgt_off, per_frame=False):
        """Waveform figures of clips already in HBM: estimate i = est_t[est_off[i]:est_off[i + 1]] against target i of
        tgt_t / tgt_off, over their common prefix -> device tensor float64 [n, hip.SCORE_FIELDS] (score.FIELDS names the
        columns); per_frame=True: -> (that, float64 [sum frames, 3] whose column 0 holds each frame's clamped segmental
        value, NaN where the frame was skipped; columns 1 - 2 are score_rows' and stay as they were allocated: NaN)."""
        n = _pair_check("score_device", est_t, est_off, tgt_t, tgt_off)
        out = torch.empty((n, hip.SCORE_FIELDS), dtype=torch.float64, device=self.device)
        fr = None
        if per_frame:
            F = sum(int(self.lib.nhans_num_frames(min(est_off[i + 1] - est_off[i], tgt_off[i + 1] - tgt_off[i]))) for i in range(n))
            fr = torch.full((F, 3), float("nan"), dtype=torch.float64, device=self.device)
        hip.check(self.lib.nhans_score_wave(self.handle, hip.ptr(est_t.contiguous()), hip.i64_array(est_off),
                                            hip.ptr(tgt_t.contiguous()), hip.i64_array(tgt_off), n, hip.ptr(out), hip.ptr(fr),
                                            self._stream()))
        return (out, fr) if per_frame else out

    def score_rows(self, est_rows_t, tgt_rows_t, frame_off, per_frame=False, frames_out=None):
        """Row figures of two float32 [rows, 201] device tensors, clip i = rows frame_off[i]:frame_off[i + 1] of both ->
        device tensor float64 [n, hip.SCORE_ROW_FIELDS] (score.ROW_FIELDS); per_frame=True: -> (that, float64 [rows, 3] with
        columns 1 - 2 = each frame's loss and lsd; frames_out: score_device's tensor, completed in place)."""
        for t in (est_rows_t, tgt_rows_t):
            if t.dim() != 2 or t.shape[1] != spec.BINS or t.dtype != torch.float32:
                raise ValueError("score_rows: float32 [n, %d] tensors" % spec.BINS)
        n = len(frame_off) - 1
        out = torch.empty((n, hip.SCORE_ROW_FIELDS), dtype=torch.float64, device=self.device)
        fr = frames_out
        if per_frame and fr is None:
            fr = torch.full((int(frame_off[-1]), 3), float("nan"), dtype=torch.float64, device=self.device)
        hip.check(self.lib.nhans_score_rows(self.handle, hip.ptr(est_rows_t.contiguous()), hip.ptr(tgt_rows_t.contiguous()),
                                            hip.i64_array(frame_off), n, hip.ptr(out), hip.ptr(fr) if per_frame else None,
                                            self._stream()))
        return (out, fr) if per_frame else out

    # ---- delay estimation (include/nhans_hip.h: nhans_align, nhans_align_cut) ------------------------
    def align_device(self, est_t, est_off, tgt_t, tgt_off, max_lag=8000, corr=False):
        """Delays of clips already in HBM: estimate i = est_t[est_off[i]:est_off[i + 1]] against target i of tgt_t / tgt_off,
        flat float32, within max_lag samples either way -> device tensor float64 [n, hip.ALIGN_FIELDS] (score.ALIGN_FIELDS
        names the columns; delay > 0: the estimate is late); corr=True: -> (that, float64 [n, 2 max_lag + 1]: the
        cross-correlation, lag -max_lag first)."""
        n, D = _pair_check("align_device", est_t, est_off, tgt_t, tgt_off), int(max_lag)
        if not 0 <= D <= hip.ALIGN_MAX_LAG:
            raise ValueError("align_device: max_lag 0 ... %d, not %r" % (hip.ALIGN_MAX_LAG, max_lag))
        out = torch.empty((n, hip.ALIGN_FIELDS), dtype=torch.float64, device=self.device)
        c = torch.empty((n, 2 * D + 1), dtype=torch.float64, device=self.device) if corr else None
        hip.check(self.lib.nhans_align(self.handle, hip.ptr(est_t.contiguous()), hip.i64_array(est_off), hip.ptr(tgt_t.contiguous()),
                                       hip.i64_array(tgt_off), n, D, hip.ptr(out), hip.ptr(c), self._stream()))
        return (out, c) if corr else out

    def align_cut_device(self, est_t, est_off, tgt_t, tgt_off, delays):
        """The pairs of align_device with their delays (host integers: column 3 of its records) taken out, in one launch ->
        (estimates, targets, offsets): two flat float32 device tensors in which pair i is [offsets[i], offsets[i + 1]), its
        n_common samples, for the scoring calls.  est_t or tgt_t may be None (its offsets still say how long its clips
        are): that signal is not cut and comes back as None -- a further signal that is sample-aligned with the target
        is cut by passing it as tgt_t with est_t=None."""
        n = len(est_off) - 1
        if len(tgt_off) - 1 != n or len(delays) != n:
            raise ValueError("align_cut_device: one target and one delay per estimate")
        for t in (est_t, tgt_t):
            if t is not None and (t.dtype != torch.float32 or t.dim() != 1):
                raise ValueError("align_cut_device: flat float32 tensors")
        d = [int(v) for v in delays]
        off = context.offsets(int(self.lib.nhans_align_common(est_off[i + 1] - est_off[i], tgt_off[i + 1] - tgt_off[i], d[i])) for i in range(n))
        ins = [None if t is None else t.contiguous() for t in (est_t, tgt_t)]
        outs = [None if t is None else torch.empty(max(off[-1], 1), dtype=torch.float32, device=self.device) for t in ins]
        hip.check(self.lib.nhans_align_cut(self.handle, hip.ptr(ins[0]), hip.i64_array(est_off), hip.ptr(ins[1]), hip.i64_array(tgt_off), n,
                                           hip.i64_array(d), hip.ptr(outs[0]), hip.ptr(outs[1]), hip.i64_array(off), self._stream()))
        return tuple(None if o is None else o[:off[-1]] for o in outs) + (off,)

    # ---- drift-aware alignment (include/nhans_hip.h: nhans_drift_track, nhans_drift_warp) -------------
    def drift_track_device(self, est_t, est_off, tgt_t, tgt_off, centres, radius=64, corr=False):
        """The delay of clips already in HBM tracked over each clip: estimate i = est_t[est_off[i]:est_off[i + 1]] against
        target i of tgt_t / tgt_off, flat float32, around the centre lines centres[i] = (ca, cb) within `radius` lags ->
        (device tensor float64 [segments, hip.DRIFT_FIELDS] -- score.DRIFT_FIELDS names the columns --, the segment
        offsets: clip i's rows are [offsets[i], offsets[i + 1])); corr=True: -> (those two, float64 [segments, 2 (radius +
        16) + 1]: each segment's lag vector, lag z - radius - 16 first)."""
        n, R = _pair_check("drift_track_device", est_t, est_off, tgt_t, tgt_off), int(radius)
        if len(centres) != n:
            raise ValueError("drift_track_device: one centre line per estimate")
        if not 1 <= R <= hip.DRIFT_MAX_RADIUS:
            raise ValueError("drift_track_device: radius 1 ... %d, not %r" % (hip.DRIFT_MAX_RADIUS, radius))
        soff = context.offsets(score_mod.drift_segments(tgt_off[i + 1] - tgt_off[i]) for i in range(n))
        S = max(soff[-1], 1)                 # (a tensor of no rows has no pointer, and the call refuses a null output)
        out = torch.empty((S, hip.DRIFT_FIELDS), dtype=torch.float64, device=self.device)
        c = torch.empty((S, 2 * (R + hip.DRIFT_TAPS) + 1), dtype=torch.float64, device=self.device) if corr else None
        hip.check(self.lib.nhans_drift_track(self.handle, hip.ptr(est_t.contiguous()), hip.i64_array(est_off), hip.ptr(tgt_t.contiguous()),
                                             hip.i64_array(tgt_off), n, hip.dbl_array(l[0] for l in centres),
                                             hip.dbl_array(l[1] for l in centres), R, hip.ptr(out), hip.ptr(c), self._stream()))
        return (out[:soff[-1]], soff, c[:soff[-1]]) if corr else (out[:soff[-1]], soff)

    def drift_warp_device(self, est_t, est_off, tgt_off, lines):
        """The estimates of drift_track_device resampled onto their targets' clocks, lines[i] = (a, b), in one launch ->
        (flat float32 device tensor, offsets, ranges): clip i's samples are [offsets[i], offsets[i + 1]) and stand for the
        target samples ranges[i] = (u_lo, u_hi) (hip.drift_range); tgt_off only says how long the targets are.  The aligned
        targets are the slices [u_lo, u_hi) -- align_cut_device with est_t=None, estimate lengths u_hi - u_lo and delays -u_lo."""
        n = len(est_off) - 1
        if len(tgt_off) - 1 != n or len(lines) != n:
            raise ValueError("drift_warp_device: one target and one line per estimate")
        if est_t.dtype != torch.float32 or est_t.dim() != 1:
            raise ValueError("drift_warp_device: a flat float32 tensor")
        rng = [hip.drift_range(est_off[i + 1] - est_off[i], tgt_off[i + 1] - tgt_off[i], lines[i][0], lines[i][1]) for i in range(n)]
        off = context.offsets(hi - lo for lo, hi in rng)
        out = torch.empty(max(off[-1], 1), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_drift_warp(self.handle, hip.ptr(est_t.contiguous()), hip.i64_array(est_off), hip.i64_array(tgt_off), n,
                                            hip.dbl_array(l[0] for l in lines), hip.dbl_array(l[1] for l in lines), hip.ptr(out),
                                            hip.i64_array(off), self._stream()))
        return out[:off[-1]], off, rng

    # ---- BSS Eval against target and interferer (include/nhans_hip.h: nhans_bss_eval) ---------------
    def bss_eval_device(self, est_t, est_off, sources, filt_len=score_mod.BSS_MAX_FILTER, filters=False):
        """SDR, SIR and SAR of clips already in HBM: estimate i = est_t[est_off[i]:est_off[i + 1]] against sources = [(tensor,
        offsets)] (the target) or [(target tensor, offsets), (interferer tensor, offsets)], flat float32, over the samples all
        of them have -> device tensor float64 [n, hip.BSS_FIELDS] (score.BSS_FIELDS names the columns); filters=True: -> (that,
        float64 [n, (J + 1) filt_len]: C, source 0's taps first, then C0)."""
        n, J, L = len(est_off) - 1, len(sources), int(filt_len)
        if J not in (1, 2) or any(len(off) - 1 != n for _, off in sources):
            raise ValueError("bss_eval_device: one or two sources, one clip of each per estimate")
        for t in [est_t] + [t for t, _ in sources]:
            if t.dtype != torch.float32 or t.dim() != 1:
                raise ValueError("bss_eval_device: flat float32 tensors")
        ten = [est_t.contiguous()] + [t.contiguous() for t, _ in sources]
        out = torch.empty((n, hip.BSS_FIELDS), dtype=torch.float64, device=self.device)
        filt = torch.empty((n, (J + 1) * L), dtype=torch.float64, device=self.device) if filters else None
        hip.check(context.bss_call(self.lib, self.handle, hip.ptr(ten[0]), [int(v) for v in est_off], [hip.ptr(t) for t in ten[1:]],
                                   [[int(v) for v in off] for _, off in sources], n, L, hip.ptr(out), hip.ptr(filt), self._stream()))
        return (out, filt) if filters else out

    # ---- STOI and extended STOI against a clean target (include/nhans_hip.h: nhans_stoi) -----------
    def stoi_device(self, est_t, est_off, tgt_t, tgt_off, rate=16000, per_segment=False):
        """STOI figures of clips already in HBM: estimate i = est_t[est_off[i]:est_off[i + 1]] against target i of tgt_t /
        tgt_off, float32 at `rate` (16000: converted to 10 kHz by nhans_stoi_resample first; 10000: as they are) -> device
        tensor float64 [n, hip.STOI_FIELDS] (score.STOI_FIELDS names the columns); per_segment=True: -> (that, float64
        [rows, 2] = d_s, e_s, the row offsets: clip i's rows begin at offsets[i] and its first `segments` are written, the
        rest stay NaN)."""
        n = _pair_check("stoi_device", est_t, est_off, tgt_t, tgt_off)
        if rate not in (16000, score_mod.STOI_RATE):
            raise ValueError("stoi_device: signals at 16000 or %d Hz, not %r" % (score_mod.STOI_RATE, rate))
        sig = [(est_t.contiguous(), [int(v) for v in est_off]), (tgt_t.contiguous(), [int(v) for v in tgt_off])]
        if rate == 16000:
            for k, (x, off) in enumerate(sig):
                o10 = context.offsets(score_mod.stoi_out_count(off[i + 1] - off[i]) for i in range(n))
                y = torch.empty(max(o10[-1], 1), dtype=torch.float32, device=self.device)
                hip.check(self.lib.nhans_stoi_resample(self.handle, hip.ptr(x), hip.i64_array(off), n, hip.ptr(y), hip.i64_array(o10),
                                                       self._stream()))
                sig[k] = (y, o10)
        (e, eo), (t, to) = sig
        out = torch.empty((n, hip.STOI_FIELDS), dtype=torch.float64, device=self.device)
        seg, soff = None, None
        if per_segment:
            soff = context.offsets(max(score_mod.stoi_num_frames(min(eo[i + 1] - eo[i], to[i + 1] - to[i])) - score_mod.STOI_SEGMENT, 0)
                                   for i in range(n))
            seg = torch.full((max(soff[-1], 1), 2), float("nan"), dtype=torch.float64, device=self.device)
        hip.check(self.lib.nhans_stoi(self.handle, hip.ptr(e), hip.i64_array(eo), hip.ptr(t), hip.i64_array(to), n, hip.ptr(out),
                                      hip.ptr(seg), self._stream()))
        return (out, seg[:soff[-1]], soff) if per_segment else out

    # ---- LLR, cepstral distance and fwSegSNR against a clean target (include/nhans_hip.h: nhans_quality) ----
    def quality_device(self, est_t, est_off, tgt_t, tgt_off, per_frame=False, bands=None):
        """The quality figures of clips already in HBM: estimate i = est_t[est_off[i]:est_off[i + 1]] against target i of
        tgt_t / tgt_off, float32 at 16 kHz -> device tensor float64 [n, hip.QUALITY_FIELDS] (score.QUALITY_FIELDS names the
        columns); per_frame=True: -> (that, float64 [frames, 3] = llr_f, cd_f, fw_f, the row offsets: clip i's rows are
        [offsets[i], offsets[i + 1]))."""
        n = _pair_check("quality_device", est_t, est_off, tgt_t, tgt_off)
        W, K = context.quality_bands_arg(bands)
        eo, to = [int(v) for v in est_off], [int(v) for v in tgt_off]
        out = torch.empty((n, hip.QUALITY_FIELDS), dtype=torch.float64, device=self.device)
        fr, foff = None, None
        if per_frame:
            foff = context.offsets(score_mod.quality_num_frames(min(eo[i + 1] - eo[i], to[i + 1] - to[i])) for i in range(n))
            fr = torch.empty((max(foff[-1], 1), 3), dtype=torch.float64, device=self.device)
        hip.check(self.lib.nhans_quality(self.handle, hip.ptr(est_t.contiguous()), hip.i64_array(eo), hip.ptr(tgt_t.contiguous()),
                                         hip.i64_array(to), n, W, K, hip.ptr(out), hip.ptr(fr), self._stream()))
        return (out, fr[:foff[-1]], foff) if per_frame else out

    # ---- mixing at a chosen SNR (include/nhans_hip.h: nhans_mix) ------------------------------------
    def mix_device(self, speech_t, speech_off, noise_t, noise_off, jobs, want=("mixture", "target", "keep", "drop")):
        """Mixtures of clips already in HBM.  jobs: (speech index, keep index or -1, drop index, snr_keep_db, snr_drop_db)
        each, the indices into speech_t / speech_off and noise_t / noise_off -> (dict of flat float32 device tensors for
        the names in `want` -- "mixture" always --, the output offsets: job j's samples are [off[j], off[j + 1]) of each,
        float64 device tensor [jobs, hip.MIX_FIELDS] whose first columns mixing.RECORD_FIELDS names)."""
        for t in (speech_t, noise_t):
            if t.dtype != torch.float32 or t.dim() != 1:
                raise ValueError("mix_device: flat float32 tensors")
        unknown = set(want) - {"mixture", "target", "keep", "drop"}
        if unknown:
            raise ValueError("mix_device: no output named %s" % sorted(unknown))
        args, off = context.mix_job_arrays(jobs, speech_off)
        out = {k: torch.empty(max(off[-1], 1), dtype=torch.float32, device=self.device)
               for k in ("mixture", "target", "keep", "drop") if k == "mixture" or k in want}
        rec = torch.empty((len(jobs), hip.MIX_FIELDS), dtype=torch.float64, device=self.device)
        hip.check(self.lib.nhans_mix(self.handle, hip.ptr(speech_t.contiguous()), hip.i64_array(speech_off), len(speech_off) - 1,
                                     hip.ptr(noise_t.contiguous()), hip.i64_array(noise_off), len(noise_off) - 1, *args, len(jobs),
                                     hip.ptr(out["mixture"]), hip.ptr(out.get("target")), hip.ptr(out.get("keep")),
                                     hip.ptr(out.get("drop")), hip.i64_array(off), hip.ptr(rec), self._stream()))
        return {k: v[:off[-1]] for k, v in out.items()}, off, rec

    def _sync(self):
        torch.cuda.current_stream(self.device).synchronize()

    # ---- whole path -------------------------------------------------------------------------
    def enhance_device(self, mix_t, mix_off, ca_t, ca_off, cb_t, cb_off, want_mixed=False, taps=False):
        """All inputs already in HBM.  Returns dict of device tensors."""
        n = len(mix_off) - 1
        nfr = [int(self.lib.nhans_num_frames(mix_off[i + 1] - mix_off[i])) for i in range(n)]
        if any(t == 0 for t in nfr):
            # (the reference dies on such a clip too: its STFT has no frames to stack)
            raise ValueError("mixture clip %d has fewer than %d samples: no STFT frame" % (nfr.index(0), spec.WIN))
        total = sum(nfr)
        res = {"denoised_wav": torch.zeros(mix_off[-1], dtype=torch.float32, device=self.device)}
        res["mixed_wav"] = torch.zeros_like(res["denoised_wav"]) if want_mixed else None
        if taps:
            for k in ("logmag", "phase", "logits"):
                res[k] = torch.empty((total, spec.BINS), dtype=torch.float32, device=self.device)
            res["emb"] = torch.empty((2 * n, spec.EMB), dtype=torch.float32, device=self.device)
        hip.check(self.lib.nhans_enhance_clips(
            self.handle, hip.ptr(mix_t), hip.i64_array(mix_off), n, hip.ptr(ca_t), hip.i64_array(ca_off),
            hip.ptr(cb_t), hip.i64_array(cb_off), hip.ptr(res["denoised_wav"]), hip.ptr(res["mixed_wav"]),
            hip.ptr(res.get("logmag")), hip.ptr(res.get("phase")), hip.ptr(res.get("logits")),
            hip.ptr(res.get("emb")), self._stream()))
        return res

    def enhance(self, mixes, ctx_a, ctx_b, want_mixed=True, taps=False, lookahead=spec.LOOKAHEAD, phase_iters=0, phase_alpha=0.0):
        """Lists of normalised float32 waveforms (mixtures trimmed) -> per-clip numpy results.  lookahead: L frames,
        0 .. 17 (include/nhans_hip.h, option "lookahead": frame g sees its clip end at g + L + 1) -- what a live stream
        of that look-ahead emits for the same samples; the saturation redo runs with the same L.  phase_iters: Griffin-Lim
        iterations (momentum phase_alpha) on the denoised rows, from the mixture's phase, before their iSTFT (option
        "phase_iters"; 0: the mixture's phase as it is); the mixed round trip and the taps stay as they are, and the redo
        runs the iterations too."""
        return self._with_phase(phase_iters, phase_alpha, lambda: self._with_lookahead(
            lookahead, lambda: self._enhance(mixes, ctx_a, ctx_b, want_mixed, taps)))

    def _enhance(self, mixes, ctx_a, ctx_b, want_mixed, taps):
        mix_t, mix_off = self._dev(mixes)
        ca_t, ca_off = self._dev(ctx_a)
        cb_t, cb_off = self._dev(ctx_b)
        res = context.redo_saturated_in_f32(
            self, lambda: self.enhance_device(mix_t, mix_off, ca_t, ca_off, cb_t, cb_off, want_mixed, taps))
        torch.cuda.synchronize(self.device)
        out = {"denoised_wav": [], "mixed_wav": []}
        den = res["denoised_wav"].cpu().numpy()
        mixed = res["mixed_wav"].cpu().numpy() if want_mixed else None
        for i in range(len(mixes)):
            out["denoised_wav"].append(den[mix_off[i]:mix_off[i + 1]])
            if want_mixed:
                out["mixed_wav"].append(mixed[mix_off[i]:mix_off[i + 1]])
        if taps:
            for k in ("logmag", "phase", "logits", "emb"):
                out[k] = res[k].cpu().numpy()
        return out

    def profile(self):
        return hip.profile_dict(self.handle)

    def profile_reset(self):
        hip.check(self.lib.nhans_profile_reset(self.handle))
