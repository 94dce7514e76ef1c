"""What every Python class over the C ABI (include/nhans_hip.h) shares, written once: the context that engine.Engine and
lite.LiteEngine both are, the f32 redo of work that saturated the f16x3 path, the device memory of either engine, and
the ragged-batch helpers.  No torch at module level: the single-process command line (lite.py) imports this."""
import ctypes
import operator
import warnings

import numpy as np

from . import hip, hiprt, mvdr as mvdr_mod, score as score_mod, spec


class Context:
    """One nhans_ctx.  A subclass's constructor sets `lib` and `handle` and says with `torch_memory` where its device
    memory and stream come from: torch (engine.Engine), or hiprt and the null stream (lite.LiteEngine)."""

    PRECISIONS = {"f32": 0, "f16x3": 1}
    torch_memory = False
    handle = None

    def set_option(self, key, value):
        hip.check(self.lib.nhans_set_option(self.handle, key.encode(), int(value)))

    def set_precision(self, precision):
        """'f32': exact f32 matrix-core path.  'f16x3': split-f16 (hi+lo, three products) on the f16
        matrix cores -- FP32-class accuracy, needs |activations| < 65504."""
        self.set_option("precision", self.PRECISIONS[precision])
        self.precision = precision

    def close(self):
        if self.handle:
            self.lib.nhans_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- activation exponents of the f16x3 mode (include/nhans_hip.h: "calibrate") ----------
    def activation_exponents(self):
        e = (ctypes.c_int * hip.NUM_ACTIVATIONS)()
        hip.check(self.lib.nhans_get_activation_exponents(self.handle, e, hip.NUM_ACTIVATIONS))
        return list(e)

    def set_activation_exponents(self, exps):
        e = (ctypes.c_int * hip.NUM_ACTIVATIONS)(*[int(v) for v in exps])
        hip.check(self.lib.nhans_set_activation_exponents(self.handle, e, hip.NUM_ACTIVATIONS))

    def activation_amax(self):
        """Largest |x| of every exponent-carrying tensor in the last finished calibration."""
        a = (ctypes.c_float * hip.NUM_ACTIVATIONS)()
        hip.check(self.lib.nhans_get_activation_amax(self.handle, a, hip.NUM_ACTIVATIONS))
        return list(a)

    def _stream(self):
        return None

    def take_status(self):
        """Waits for the current stream; returns and clears the sticky device status bits
        (hip.STATUS_SATURATED: a split-f16 activation did not fit f16 and was clamped)."""
        flags = ctypes.c_int(0)
        hip.check(self.lib.nhans_take_status(self.handle, ctypes.byref(flags), self._stream()))
        return flags.value

    def _with_lookahead(self, L, run):
        """run() with the option "lookahead" at L frames and back at the default afterwards, whatever run() did."""
        if L == spec.LOOKAHEAD:
            return run()
        spec.check_lookahead(L)
        self.set_option("lookahead", L)
        try:
            return run()
        finally:
            self.set_option("lookahead", spec.LOOKAHEAD)

    def _with_phase(self, iters, alpha, run):
        """run() with the option "phase_iters" at `iters` Griffin-Lim iterations of momentum `alpha` (include/nhans_hip.h:
        nhans_phase_*) and back at none afterwards, whatever run() did."""
        if not iters:
            return run()
        if not 0 < int(iters) <= hip.PHASE_MAX_ITERS:
            raise ValueError("phase_iters 0 ... %d, not %r" % (hip.PHASE_MAX_ITERS, iters))
        hip.check(self.lib.nhans_phase_set_alpha(self.handle, float(alpha)))
        self.set_option("phase_iters", int(iters))
        try:
            return run()
        finally:
            self.set_option("phase_iters", 0)
            hip.check(self.lib.nhans_phase_set_alpha(self.handle, 0.0))

    # ---- filterbank features of the enhanced clips (include/nhans_hip.h: nhans_fbank_*) --------
    def features(self, mixes, ctx_a, ctx_b, fb, lookahead=spec.LOOKAHEAD, mixed=False):
        """Lists of normalised float32 waveforms (mixtures trimmed, as enhance takes them) -> one float32 [T_i, fb.n_mels]
        array per clip: fb (fbank.Filterbank) applied to the clip's denoised log-magnitude rows -- STFT, tower, stack and
        filterbank on the device, no iSTFT, and only the features come back.  Frame g is centred on sample 160 g + 200.
        lookahead as in enhance: what a live stream of that look-ahead computes for the same samples, bit for bit.
        mixed=True: -> (denoised features, features of the unprocessed rows), two such lists.  The saturation redo of
        enhance applies here too."""
        return self._with_lookahead(lookahead, lambda: self._features(mixes, ctx_a, ctx_b, fb, mixed))

    def _features(self, mixes, ctx_a, ctx_b, fb, mixed):
        if not (len(mixes) == len(ctx_a) == len(ctx_b)):
            raise ValueError("features: one (a, b) pair of conditioning recordings per clip")
        lib, mem, n = self.lib, Mem(self), len(mixes)
        (mf, off), (af, aoff), (bf, boff) = flat(mixes), flat(ctx_a), flat(ctx_b)
        nfr = [int(lib.nhans_num_frames(off[i + 1] - off[i])) for i in range(n)]
        if any(t == 0 for t in nfr):
            raise ValueError("mixture clip %d has fewer than %d samples: no STFT frame" % (nfr.index(0), spec.WIN))
        foff = offsets(nfr)
        T, nm = foff[-1], fb.n_mels
        h, s = fb.handle(self), mem.stream()
        ins = [mem.up(x) for x in (mf, af, bf)]
        lm, den = mem.empty(T * spec.BINS), mem.empty(T * spec.BINS)
        ctx_lm, emb = mem.empty(2 * n * spec.NOISE_WIN * spec.BINS), mem.empty(2 * n * spec.EMB)
        out = [mem.empty(T * nm), mem.empty(T * nm) if mixed else None]

        def at(buf, floats):
            return ctypes.c_void_p(mem.p(buf).value + 4 * floats)

        def run():
            c = hip.check
            c(lib.nhans_stft_features(self.handle, mem.p(ins[0]), hip.i64_array(off), n, 0, mem.p(lm), None, s))
            c(lib.nhans_stft_features(self.handle, mem.p(ins[1]), hip.i64_array(aoff), n, spec.NOISE_WIN, mem.p(ctx_lm), None, s))
            c(lib.nhans_stft_features(self.handle, mem.p(ins[2]), hip.i64_array(boff), n, spec.NOISE_WIN,
                                      at(ctx_lm, n * spec.NOISE_WIN * spec.BINS), None, s))
            c(lib.nhans_embed(self.handle, mem.p(ctx_lm), 2 * n, mem.p(emb), s))
            c(lib.nhans_mask_net(self.handle, mem.p(lm), hip.i64_array(foff), n, mem.p(emb), at(emb, n * spec.EMB), None,
                                 mem.p(den), s))
            c(lib.nhans_fbank_rows(h, mem.p(den), T, mem.p(out[0]), s))
            if mixed:
                c(lib.nhans_fbank_rows(h, mem.p(lm), T, mem.p(out[1]), s))

        try:
            redo_saturated_in_f32(self, run)          # (take_status waits for the stream)
            res = [np.array(mem.down(o, T * nm), dtype=np.float32).reshape(T, nm) if o is not None else None for o in out]
        finally:
            mem.free(*ins, lm, den, ctx_lm, emb, *out)
        split = [[r[foff[i]:foff[i + 1]] for i in range(n)] if r is not None else None for r in res]
        return (split[0], split[1]) if mixed else split[0]


    # ---- scoring against a clean target (include/nhans_hip.h: nhans_score_*) ---------------------
    def score(self, estimates, targets, per_frame=False, stoi=False, bss=None, align=None, delays=None, quality=False, drift=False):
        """Lists of float32 waveforms, estimate i against target i over their common prefix -> one dict per clip: the
        waveform figures (score.FIELDS: si_sdr_db, snr_db, segsnr_db, ...) and the row figures loss and lsd_db of the two
        signals' own log-magnitude rows (nhans_stft_features) -- one upload, two STFTs and the two score calls on the
        device, one download of the records.  per_frame=True: plus "per_frame", float64 [frames, 3]: each frame's clamped
        segmental value (NaN where its target is silent), loss and lsd.  stoi=True: plus the figures of Context.stoi of
        the same pairs (16 kHz signals), merged into each record -- a name the record already has (n, frames: there the
        16 kHz samples and the STFT rows) is prefixed: stoi_n, stoi_frames.  bss: a list of interferers (or True: the
        target alone) -- plus the figures of Context.bss_eval of the same estimates (sdr_db, sir_db, sar_db, ...), merged
        into each record; its n is bss_n.  quality=True: plus the figures of Context.quality of the same pairs (llr, llr_95,
        cd_db, cd_95_db, fwsegsnr_db, frames_lpc, frames_fw), merged into each record; its n and frames are quality_n and
        quality_frames.
        Signals that are not aligned: align=D estimates one delay per pair within D samples either way (Context.align),
        delays=[...] applies given integers (positive: the estimate is late); each pair is cut to its common part
        (score.align_cut; an interferer as its target) and scored as above, and each record gains "delay" and, where the
        delay was estimated, "align_rho".
        Signals sampled by two clocks: align=D with drift=True fits a line to the delay over the clip (Context.align_drift)
        and resamples the estimate onto the target's clock (Context.drift_warp; the target and an interferer are cut to
        the warp's range); each record gains "delay" (real, at the target's first sample), "drift_ppm", "drift_ok" and
        "align_rho".  A pair without a good fit (drift_ok 0) is cut by its whole-sample delay, exactly as without drift."""
        if len(estimates) != len(targets):
            raise ValueError("score: one target per estimate")
        if drift:
            if align is None:
                raise ValueError("score: drift=True tracks the delay around the one align=D estimates: give align=")
            extra = bss if bss is not None and bss is not False and bss is not True else None
            if extra is not None and len(extra) != len(estimates):
                raise ValueError("score: one interferer per estimate")
            lines = self.align_drift(estimates, targets, max_lag=align)
            es, ts, xs = self._drift_pairs(estimates, targets, extra, lines)
            recs = self.score(es, ts, per_frame=per_frame, stoi=stoi, bss=xs if extra is not None else bss, quality=quality)
            return [dict(r, delay=l["delay"] if l["fit_ok"] else l["delay_int"], drift_ppm=l["drift_ppm"], drift_ok=l["fit_ok"],
                         align_rho=l["rho"]) for r, l in zip(recs, lines)]
        if align is not None or delays is not None:
            extra = bss if bss is not None and bss is not False and bss is not True else None
            es, ts, xs, tags = self._aligned("score", estimates, targets, extra, align, delays)
            recs = self.score(es, ts, per_frame=per_frame, stoi=stoi, bss=xs if extra is not None else bss, quality=quality)
            return [dict(r, **tag) for r, tag in zip(recs, tags)]
        if quality:
            return [score_mod.merge_quality(r, qr)
                    for r, qr in zip(self.score(estimates, targets, per_frame=per_frame, stoi=stoi, bss=bss),
                                     self.quality(estimates, targets))]
        if bss is not None and bss is not False:
            return [score_mod.merge_bss(r, b)
                    for r, b in zip(self.score(estimates, targets, per_frame=per_frame, stoi=stoi),
                                    self.bss_eval(estimates, targets, None if bss is True else bss))]
        if stoi:
            return [score_mod.merge_stoi(r, t)
                    for r, t in zip(self.score(estimates, targets, per_frame=per_frame), self.stoi(estimates, targets))]
        lib, mem, n = self.lib, Mem(self), len(estimates)
        cut = [min(len(e), len(t)) for e, t in zip(estimates, targets)]
        (ef, off), (tf, _) = flat([e[:k] for e, k in zip(estimates, cut)]), flat([t[:k] for t, k in zip(targets, cut)])
        foff = offsets(int(lib.nhans_num_frames(k)) for k in cut)
        F, nw, nr = foff[-1], hip.SCORE_FIELDS, hip.SCORE_ROW_FIELDS
        s = mem.stream()
        ins = [mem.up(ef), mem.up(tf)]
        lm = [mem.empty(F * spec.BINS), mem.empty(F * spec.BINS)]
        out = mem.empty(n * (nw + nr) + 3 * F, np.float64)

        def at(doubles):
            return ctypes.c_void_p(mem.p(out).value + 8 * doubles)

        fr = at(n * (nw + nr)) if per_frame else None
        try:
            if n:
                o = hip.i64_array(off)
                if F:
                    for x, rows in zip(ins, lm):
                        hip.check(lib.nhans_stft_features(self.handle, mem.p(x), o, n, 0, mem.p(rows), None, s))
                hip.check(lib.nhans_score_wave(self.handle, mem.p(ins[0]), o, mem.p(ins[1]), o, n, at(0), fr, s))
                hip.check(lib.nhans_score_rows(self.handle, mem.p(lm[0]), mem.p(lm[1]), hip.i64_array(foff), n, at(n * nw), fr, s))
            self._sync()
            got = np.array(mem.down(out, n * (nw + nr) + 3 * F, np.float64), dtype=np.float64)
        finally:
            mem.free(*ins, *lm, out)
        res = []
        for i in range(n):
            rec = score_mod.record(got[i * nw:(i + 1) * nw])
            rec.update(score_mod.row_record(got[n * nw + i * nr:n * nw + (i + 1) * nr]))
            if per_frame:
                rec["per_frame"] = got[n * (nw + nr):].reshape(F, 3)[foff[i]:foff[i + 1]].copy()
            res.append(rec)
        return res

    # ---- delay estimation (include/nhans_hip.h: nhans_align) ---------------------------------------
    def align(self, estimates, targets, max_lag=8000, corr=False):
        """Lists of float32 waveforms, estimate i against target i -> one dict per clip by score.ALIGN_FIELDS: delay (the lag
        within max_lag samples either way at which the cross-correlation is largest; positive: the estimate is late,
        e[u + delay] lines up with t[u]), rho (that value over the root of the two energies), c_peak, n_common, ne, nt, D.
        One upload, one call, one download.  corr=True: plus "corr", float64 [2 max_lag + 1], lag -max_lag first."""
        if len(estimates) != len(targets):
            raise ValueError("align: one target per estimate")
        n, D = len(estimates), int(max_lag)
        (ef, eoff), (tf, toff) = flat(estimates), flat(targets)
        nf, per = hip.ALIGN_FIELDS, (2 * D + 1 if corr else 0)
        got = self._records_call([ef, tf], n * nf, n * per if corr else None, lambda at, out, extra, s: self.lib.nhans_align(
            self.handle, at(0), hip.i64_array(eoff), at(1), hip.i64_array(toff), n, D, out, extra, s))
        res = []
        for i in range(n):
            rec = score_mod.align_record(got[i * nf:(i + 1) * nf])
            if corr:
                rec["corr"] = got[n * nf + i * per:n * nf + (i + 1) * per].copy()
            res.append(rec)
        return res

    def _aligned(self, who, estimates, targets, others, align, delays):
        """The pairs with their delays taken out -> (estimates, targets, others, what each record gains): align=D
        estimates the delays (Context.align), delays=[...] are given; `others` (None, or one further signal per pair that
        is sample-aligned with its target) are cut as the targets are."""
        if align is not None and delays is not None:
            raise ValueError("%s: align= estimates the delays and delays= gives them: not both" % who)
        if others is not None and len(others) != len(estimates):
            raise ValueError("%s: one interferer per estimate" % who)
        if align is not None:
            recs = self.align(estimates, targets, max_lag=align)
            tags = [{"delay": r["delay"], "align_rho": r["rho"]} for r in recs]
        else:
            if len(delays) != len(estimates):
                raise ValueError("%s: one delay per estimate" % who)
            tags = [{"delay": int(d)} for d in delays]
        pairs = [score_mod.align_cut(e, t, tag["delay"]) for e, t, tag in zip(estimates, targets, tags)]
        xs = None if others is None else [score_mod.align_cut(e, x, tag["delay"])[1] for e, x, tag in zip(estimates, others, tags)]
        return [p[0] for p in pairs], [p[1] for p in pairs], xs, tags

    # ---- drift-aware alignment (include/nhans_hip.h: nhans_drift_*) --------------------------------
    def drift_track(self, estimates, targets, centres, radius=64, corr=False):
        """Lists of float32 waveforms, estimate i against target i, tracked in blocks of 4,096 target samples at hop 2,048
        around the centre lines centres[i] = (ca, cb) within `radius` lags -> per clip a list of one dict per segment by
        score.DRIFT_FIELDS: u (the block's energy centroid), tau (the delay there), rho, E_t, v_peak, d_int, flags, z.  One
        upload, one launch, one download.  corr=True: each segment plus "corr", float64 [2 (radius + 16) + 1], lag
        z - radius - 16 first."""
        if len(estimates) != len(targets) or len(centres) != len(estimates):
            raise ValueError("drift_track: one target and one centre line per estimate")
        n, R = len(estimates), int(radius)
        (ef, eoff), (tf, toff) = flat(estimates), flat(targets)
        soff = offsets(score_mod.drift_segments(len(t)) for t in targets)
        S, nf, per = soff[-1], hip.DRIFT_FIELDS, 2 * (R + hip.DRIFT_TAPS) + 1
        ca, cb = hip.dbl_array(c[0] for c in centres), hip.dbl_array(c[1] for c in centres)
        got = self._records_call([ef, tf], S * nf, S * per if corr else None, lambda at, out, extra, s: self.lib.nhans_drift_track(
            self.handle, at(0), hip.i64_array(eoff), at(1), hip.i64_array(toff), n, ca, cb, R, out, extra, s))
        res = []
        for i in range(n):
            segs = []
            for k in range(soff[i], soff[i + 1]):
                rec = score_mod.drift_segment_record(got[k * nf:(k + 1) * nf])
                if corr:
                    rec["corr"] = got[S * nf + k * per:S * nf + (k + 1) * per].copy()
                segs.append(rec)
            res.append(segs)
        return res

    def drift_warp(self, estimates, target_lengths, lines):
        """Lists of float32 waveforms, the lengths of their targets and one line (a, b) each -> per clip (y, u_lo, u_hi): the
        estimate resampled onto the target's clock, y[u - u_lo] = the estimate at a + u + b u for the u of [u_lo, u_hi) --
        the largest range of the target whose positions lie inside the estimate (hip.drift_range).  The aligned target
        is target[u_lo:u_hi].  One upload, one launch, one download."""
        if len(target_lengths) != len(estimates) or len(lines) != len(estimates):
            raise ValueError("drift_warp: one target length and one line per estimate")
        lib, mem, n = self.lib, Mem(self), len(estimates)
        ef, eoff = flat(estimates)
        toff = offsets(target_lengths)
        rng = [hip.drift_range(eoff[i + 1] - eoff[i], toff[i + 1] - toff[i], lines[i][0], lines[i][1]) for i in range(n)]
        ooff = offsets(hi - lo for lo, hi in rng)
        buf, out = mem.up(ef), mem.empty(ooff[-1])
        try:
            hip.check(lib.nhans_drift_warp(self.handle, mem.p(buf), hip.i64_array(eoff), hip.i64_array(toff), n,
                                           hip.dbl_array(l[0] for l in lines), hip.dbl_array(l[1] for l in lines), mem.p(out),
                                           hip.i64_array(ooff), mem.stream()))
            self._sync()
            got = np.array(mem.down(out, ooff[-1]), dtype=np.float32)
        finally:
            mem.free(buf, out)
        return [(got[ooff[i]:ooff[i + 1]], rng[i][0], rng[i][1]) for i in range(n)]

    def drift_fit(self, segments, rho_min=score_mod.DRIFT_RHO_MIN, trim=score_mod.DRIFT_TRIM):
        """The line through one clip's segments (drift_track's dicts): nhans_drift_fit -> dict by score.DRIFT_FIT_FIELDS."""
        return hip.drift_fit([[s[k] for k in score_mod.DRIFT_FIELDS] for s in segments], rho_min, trim)

    def align_drift(self, estimates, targets, max_lag=8000, track_lag=64):
        """Lists of float32 waveforms, estimate i against target i -> one dict per pair: the line p(u) = delay + u + drift u of
        the estimate's positions over the target's samples u.  Context.align gives the whole-sample delay d0 within max_lag;
        the delay is tracked over the clip around (d0, 0) within track_lag lags and a line fitted (drift_track, drift_fit);
        where that fit is good the clip is tracked again around the fitted line within 8 lags -- which recovers the outer
        segments of a long clip, whose delay has left the first window -- and fitted again.  Keys: delay (real, samples at
        u = 0; positive: the estimate is late), drift (b) and drift_ppm (10^6 b; positive: the estimate's clock runs fast),
        fit_ok, segments, segments_used, rms_residual, rho (of the whole-sample record), delay_int (d0).  Where fit_ok is 0
        -- a clip of fewer than three blocks, too few segments that correlate, a slope beyond 2^-10 -- delay is d0 and drift 0.
        segments_used and rms_residual are those of the last fit made, whether it was good or not: where the first fit was
        good and the second was not, they describe the second, failed one, and the result is still (d0, 0)."""
        coarse = self.align(estimates, targets, max_lag=max_lag)
        n = len(coarse)
        fits = [self.drift_fit(s) for s in self.drift_track(estimates, targets, [(float(r["delay"]), 0.0) for r in coarse], radius=track_lag)]
        again = [i for i in range(n) if fits[i]["fit_ok"]]
        if again:
            segs = self.drift_track([estimates[i] for i in again], [targets[i] for i in again],
                                    [(fits[i]["a"], fits[i]["b"]) for i in again], radius=8)
            for i, s in zip(again, segs):
                fits[i] = self.drift_fit(s)
        res = []
        for r, f in zip(coarse, fits):
            ok = bool(f["fit_ok"])
            a, b = (f["a"], f["b"]) if ok else (float(r["delay"]), 0.0)
            res.append({"delay": a, "drift": b, "drift_ppm": 1e6 * b, "fit_ok": int(ok), "segments": score_mod.drift_segments(r["nt"]),
                        "segments_used": f["n_used"], "rms_residual": f["rms_residual"], "rho": r["rho"], "delay_int": r["delay"]})
        return res

    def _drift_pairs(self, estimates, targets, others, lines):
        """The pairs with their lines (align_drift's dicts) taken out -> (estimates, targets, others): a pair whose fit is good
        is warped onto the target's clock (drift_warp) and its target -- and the further signal of `others` that is
        sample-aligned with it -- cut to the warp's range; any other pair is cut by its whole-sample delay (score.align_cut)."""
        ok = [i for i, l in enumerate(lines) if l["fit_ok"]]
        warped = dict(zip(ok, self.drift_warp([estimates[i] for i in ok], [len(targets[i]) for i in ok],
                                              [(lines[i]["delay"], lines[i]["drift"]) for i in ok]))) if ok else {}
        es, ts, xs = [], [], (None if others is None else [])
        for i, (e, t) in enumerate(zip(estimates, targets)):
            if i in warped:
                y, lo, hi = warped[i]
                cut = lambda x: x[lo:hi]
            else:
                d = lines[i]["delay_int"]
                y = score_mod.align_cut(e, t, d)[0]
                cut = lambda x, d=d: score_mod.align_cut(e, x, d)[1]
            es.append(y)
            ts.append(cut(t))
            if others is not None:
                xs.append(cut(others[i]))
        return es, ts, xs

    # ---- STOI and extended STOI against a clean target (include/nhans_hip.h: nhans_stoi) ----------
    def stoi(self, estimates, targets, rate=16000, per_segment=False, delays=None):
        """Lists of float32 waveforms at `rate` (16000: the network's, converted to 10 kHz on the device by
        nhans_stoi_resample; 10000: scored as they are), estimate i against target i -> one dict per clip by
        score.STOI_FIELDS: n (common samples at 10 kHz), frames, frames_kept, segments, stoi, estoi -- NaN for both figures
        where there is no segment.  One upload, the conversion, the score and one download of the records.
        per_segment=True: plus "per_segment", float64 [segments, 2] = each segment's d_s and e_s.  delays=[...]: each pair
        is first cut to its common part with the estimate's delay (samples at `rate`, positive: late) taken out, and each
        record gains "delay"."""
        if len(estimates) != len(targets):
            raise ValueError("stoi: one target per estimate")
        if delays is not None:
            es, ts, _, tags = self._aligned("stoi", estimates, targets, None, None, delays)
            return [dict(r, **tag) for r, tag in zip(self.stoi(es, ts, rate=rate, per_segment=per_segment), tags)]
        if rate not in (16000, score_mod.STOI_RATE):
            raise ValueError("stoi: signals at 16000 or %d Hz, not %r" % (score_mod.STOI_RATE, rate))
        lib, mem, n = self.lib, Mem(self), len(estimates)
        (ef, eoff), (tf, toff) = flat(estimates), flat(targets)
        s = mem.stream()
        bufs = [mem.up(ef), mem.up(tf)]
        offs = [eoff, toff]
        try:
            if rate == 16000 and n:
                for k in (0, 1):
                    o10 = offsets(score_mod.stoi_out_count(offs[k][i + 1] - offs[k][i]) for i in range(n))
                    conv = mem.empty(o10[-1])
                    bufs.append(conv)
                    hip.check(lib.nhans_stoi_resample(self.handle, mem.p(bufs[k]), hip.i64_array(offs[k]), n, mem.p(conv),
                                                      hip.i64_array(o10), s))
                    offs[k] = o10
                src = bufs[2:]
            else:
                src = bufs[:2]
            cnt = [min(offs[0][i + 1] - offs[0][i], offs[1][i + 1] - offs[1][i]) for i in range(n)]
            soff = offsets(max(score_mod.stoi_num_frames(k) - score_mod.STOI_SEGMENT, 0) for k in cnt)
            nf, ns = hip.STOI_FIELDS, soff[-1] if per_segment else 0
            out = mem.empty(n * nf + 2 * ns, np.float64)
            bufs.append(out)
            if n:
                seg = ctypes.c_void_p(mem.p(out).value + 8 * n * nf) if per_segment else None
                hip.check(lib.nhans_stoi(self.handle, mem.p(src[0]), hip.i64_array(offs[0]), mem.p(src[1]), hip.i64_array(offs[1]), n,
                                         mem.p(out), seg, s))
            self._sync()
            got = np.array(mem.down(out, n * nf + 2 * ns, np.float64), dtype=np.float64)
        finally:
            mem.free(*bufs)
        res = []
        for i in range(n):
            rec = score_mod.stoi_record(got[i * nf:(i + 1) * nf])
            if per_segment:
                rec["per_segment"] = got[n * nf:].reshape(ns, 2)[soff[i]:soff[i] + rec["segments"]].copy()
            res.append(rec)
        return res

    # ---- LLR, cepstral distance and fwSegSNR against a clean target (include/nhans_hip.h: nhans_quality) ----
    def quality(self, estimates, targets, per_frame=False, bands=None, delays=None):
        """Lists of float32 waveforms at 16 kHz, estimate i against target i over their common prefix -> one dict per clip by
        score.QUALITY_FIELDS: n, frames, frames_lpc, frames_fw, llr, llr_95, cd_db, cd_95_db (lower is better for these
        four) and fwsegsnr_db -- NaN where no frame was kept.  One upload, one call, one download.  per_frame=True: plus
        "per_frame", float64 [frames, 3] = each frame's llr_f, cd_f and fw_f, NaN where it was skipped.  bands: a
        non-negative [K <= 32, 257] matrix in place of score.quality_band_matrix().  delays=[...]: each pair is first cut
        to its common part with the estimate's delay (positive: late) taken out, and each record gains "delay"."""
        if len(estimates) != len(targets):
            raise ValueError("quality: one target per estimate")
        if delays is not None:
            es, ts, _, tags = self._aligned("quality", estimates, targets, None, None, delays)
            return [dict(r, **tag) for r, tag in zip(self.quality(es, ts, per_frame=per_frame, bands=bands), tags)]
        n, nf = len(estimates), hip.QUALITY_FIELDS
        W, K = quality_bands_arg(bands)
        (ef, eoff), (tf, toff) = flat(estimates), flat(targets)
        foff = offsets(score_mod.quality_num_frames(min(eoff[i + 1] - eoff[i], toff[i + 1] - toff[i])) for i in range(n))
        got = self._records_call([ef, tf], n * nf, 3 * foff[-1] if per_frame else None, lambda at, out, extra, s: self.lib.nhans_quality(
            self.handle, at(0), hip.i64_array(eoff), at(1), hip.i64_array(toff), n, W, K, out, extra, s))
        res = []
        for i in range(n):
            rec = score_mod.quality_record(got[i * nf:(i + 1) * nf])
            if per_frame:
                rec["per_frame"] = got[n * nf:].reshape(-1, 3)[foff[i]:foff[i + 1]].copy()
            res.append(rec)
        return res

    def quality_lpc(self, estimates, targets):
        """The per-frame LPC quantities of nhans_quality (nhans_quality_lpc; for tests and diagnosis) -> one float64
        [frames, hip.QUALITY_LPC_FIELDS] array per clip: r_t[17], r_e[17], a_t[17], a_e[17], num, den, dc2, 0."""
        if len(estimates) != len(targets):
            raise ValueError("quality_lpc: one target per estimate")
        n, nl = len(estimates), hip.QUALITY_LPC_FIELDS
        (ef, eoff), (tf, toff) = flat(estimates), flat(targets)
        foff = offsets(score_mod.quality_num_frames(min(eoff[i + 1] - eoff[i], toff[i + 1] - toff[i])) for i in range(n))
        got = self._records_call([ef, tf], nl * foff[-1], None, lambda at, out, extra, s: self.lib.nhans_quality_lpc(
            self.handle, at(0), hip.i64_array(eoff), at(1), hip.i64_array(toff), n, out, s)).reshape(-1, nl)
        return [got[foff[i]:foff[i + 1]].copy() for i in range(n)]

    # ---- BSS Eval against target and interferer (include/nhans_hip.h: nhans_bss_eval) -------------
    def bss_eval(self, estimates, targets, interferers=None, filt_len=score_mod.BSS_MAX_FILTER, filters=False, delays=None):
        """Lists of float32 waveforms, estimate i against target i and (interferers given) interferer i over the samples
        all of them have -> one dict per clip by score.BSS_FIELDS: sdr_db, sir_db, sar_db, the six energies, n, J, L and
        singular (1: the Gram matrix failed the pivot rule -- an all-zero source, say -- and every figure is NaN).  One
        upload, one call, one download.  filters=True: plus "C", float64 [J, filt_len], and "C0", float64 [filt_len].
        delays=[...]: each tuple is first cut to its common part with the estimate's delay (positive: late) taken out --
        the interferer as its target -- and each record gains "delay"."""
        src = [targets] if interferers is None else [targets, interferers]
        if any(len(s) != len(estimates) for s in src):
            raise ValueError("bss_eval: one target%s per estimate" % ("" if interferers is None else " and one interferer"))
        if delays is not None:
            es, ts, xs, tags = self._aligned("bss_eval", estimates, targets, interferers, None, delays)
            return [dict(r, **tag) for r, tag in zip(self.bss_eval(es, ts, xs, filt_len=filt_len, filters=filters), tags)]
        n, J, L = len(estimates), len(src), int(filt_len)
        flats = [flat(x) for x in [estimates] + src]
        nf, per = hip.BSS_FIELDS, (J + 1) * L if filters else 0
        got = self._records_call([f for f, _ in flats], n * nf, n * per if filters else None, lambda at, out, extra, s: bss_call(
            self.lib, self.handle, at(0), flats[0][1], [at(1 + j) for j in range(J)], [flats[1 + j][1] for j in range(J)], n, L, out, extra, s))
        res = []
        for i in range(n):
            rec = score_mod.bss_record(got[i * nf:(i + 1) * nf])
            if filters:
                f = got[n * nf + i * per:n * nf + (i + 1) * per]
                rec.update(C=f[:J * L].reshape(J, L).copy(), C0=f[J * L:].copy())
            res.append(rec)
        return res

    # ---- mixing at a chosen SNR (include/nhans_hip.h: nhans_mix) -----------------------------------
    def mix(self, speech, noises, jobs):
        """Lists of float32 recordings and jobs (speech index, keep index or -1, drop index, snr_keep_db, snr_drop_db) ->
        (dict "mixture" / "target" / "keep" / "drop" -> one float32 array per job, one record dict per job by
        mixing.RECORD_FIELDS): mixing.domixing -- without a keep noise mixing.domixing_separator -- of every job, bit for
        bit, computed on the device: one upload, the three launches, one download.  The indices let one triple of
        recordings serve many SNR pairs; a power is computed once per distinct (recording, fitted length)."""
        from . import mixing
        lib, mem, nj = self.lib, Mem(self), len(jobs)
        (sf, soff), (nf, noff) = flat(speech), flat(noises)
        args, off = mix_job_arrays(jobs, soff)
        names = ("mixture", "target", "keep", "drop")
        ins = [mem.up(sf), mem.up(nf)]
        outs = [mem.empty(off[-1]) for _ in names]
        rec = mem.empty(nj * hip.MIX_FIELDS, np.float64)
        try:
            hip.check(lib.nhans_mix(self.handle, mem.p(ins[0]), hip.i64_array(soff), len(speech), mem.p(ins[1]), hip.i64_array(noff),
                                    len(noises), *args, nj, *[mem.p(o) for o in outs], hip.i64_array(off), mem.p(rec), mem.stream()))
            self._sync()
            got = [np.array(mem.down(o, off[-1]), dtype=np.float32) for o in outs]
            recs = np.array(mem.down(rec, nj * hip.MIX_FIELDS, np.float64), dtype=np.float64).reshape(nj, hip.MIX_FIELDS)
        finally:
            mem.free(*ins, *outs, rec)
        signals = {k: [g[off[j]:off[j + 1]] for j in range(nj)] for k, g in zip(names, got)}
        return signals, [dict(zip(mixing.RECORD_FIELDS, (float(v) for v in r))) for r in recs]

    # ---- mask-driven MVDR beamforming (include/nhans_hip.h: nhans_mvdr_*) ---------------------------
    def _array_clips(self, who, clips):
        """[n_i, C] arrays -> (the float32 arrays, C, the flat planes of all clips, the per-channel sample offsets, the
        frame offsets); every clip has a frame."""
        xs = [np.asarray(x, dtype=np.float32) for x in clips]
        if not xs or any(x.ndim != 2 for x in xs) or len({x.shape[1] for x in xs}) != 1:
            raise ValueError("%s: a list of [n, C] arrays of one channel count C" % who)
        C = xs[0].shape[1]
        if not 1 <= C <= hip.MVDR_MAX_CHANNELS:
            raise ValueError("%s: 1 ... %d channels, not %d" % (who, hip.MVDR_MAX_CHANNELS, C))
        off = offsets(len(x) for x in xs)
        nfr = [int(self.lib.nhans_num_frames(len(x))) for x in xs]
        if any(t == 0 for t in nfr):
            raise ValueError("%s: clip %d has fewer than %d samples: no STFT frame" % (who, nfr.index(0), spec.WIN))
        pf = np.ascontiguousarray(np.concatenate([mvdr_mod.planes(x) for x in xs]))
        return xs, C, pf, off, offsets(nfr)

    def mvdr(self, clips, masks, ref=0, loading=mvdr_mod.LOADING, loggain=False, gains=None, stages=False):
        """Lists of [n_i, C] float32 clips (one C) and of [T_i, 201] mask rows -- loggain=True: log-gain rows, what mask_net
        writes as logits -- -> one dict per clip: "logmag" and "phase", float32 [T_i, 201]: the rows of the beamformed
        signal y = w^H x (gains: a list of [T_i, 201] log-gains added to logmag); "w", complex128 [201, C]; "record" by
        mvdr.FIELDS.  One upload, nhans_mvdr, one download.  stages=True: the three stage calls instead (the same bits),
        and each dict gains "y" complex64 [T_i, 201] (the beamformed values before any gain), "X" complex64 [C, T_i, 201], "phi_s" and "phi_n" complex128 [201, C, C], and "chan_logmag" and
        "chan_phase", float32 [C, T_i, 201]: the analysis rows of every channel."""
        xs, C, pf, off, foff = self._array_clips("mvdr", clips)
        n, F, B = len(xs), foff[-1], spec.BINS
        rows_of = lambda lst: np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1) for r in lst]))
        for lst in (masks, gains):
            if lst is not None and (len(lst) != n or any(np.shape(r) != (foff[i + 1] - foff[i], B) for i, r in enumerate(lst))):
                raise ValueError("mvdr: one [T_i, %d] array of rows per clip" % B)
        lib, mem = self.lib, Mem(self)
        flags = hip.MVDR_LOGGAIN if loggain else 0
        nf = hip.MVDR_FIELDS
        ins = [mem.up(pf), mem.up(rows_of(masks)), mem.up(rows_of(gains)) if gains is not None else None]
        lm, ph = mem.empty(F * B), mem.empty(F * B)
        w, rec = mem.empty(n * B * C * 2, np.float64), mem.empty(n * nf, np.float64)
        X = cov = clm = cph = yb = None
        if stages:
            X, clm, cph = mem.empty(2 * C * F * B), mem.empty(C * F * B), mem.empty(C * F * B)
            cov, yb = mem.empty(n * 4 * C * C * B, np.float64), mem.empty(2 * F * B)
        try:
            s, so, fo = mem.stream(), hip.i64_array(off), hip.i64_array(foff)
            if stages:
                hip.check(lib.nhans_mvdr_spectra(self.handle, mem.p(ins[0]), so, n, C, mem.p(X), mem.p(clm), mem.p(cph), s))
                hip.check(lib.nhans_mvdr_weights(self.handle, mem.p(X), mem.p(ins[1]), fo, n, C, int(ref), float(loading), flags,
                                                 mem.p(w), mem.p(cov), mem.p(rec), s))
                hip.check(lib.nhans_mvdr_apply(self.handle, mem.p(X), mem.p(w), mem.p(ins[2]), fo, n, C, mem.p(lm), mem.p(ph),
                                               mem.p(yb), mem.p(rec), s))
            else:
                hip.check(lib.nhans_mvdr(self.handle, mem.p(ins[0]), so, n, C, mem.p(ins[1]), int(ref), float(loading), flags,
                                         mem.p(ins[2]), mem.p(lm), mem.p(ph), mem.p(w), mem.p(rec), s))
            self._sync()
            g = lambda buf, cnt, dt=np.float32: np.array(mem.down(buf, cnt, dt), dtype=dt)
            lm_h, ph_h = g(lm, F * B).reshape(F, B), g(ph, F * B).reshape(F, B)
            w_h = g(w, n * B * C * 2, np.float64).view(np.complex128).reshape(n, B, C)
            rec_h = g(rec, n * nf, np.float64).reshape(n, nf)
            if stages:
                X_h = g(X, 2 * C * F * B).view(np.complex64).reshape(C * F, B)
                clm_h, cph_h = g(clm, C * F * B).reshape(C * F, B), g(cph, C * F * B).reshape(C * F, B)
                cov_h = g(cov, n * 4 * C * C * B, np.float64).view(np.complex128).reshape(n, 2, C, C, B)
                y_h = g(yb, 2 * F * B).view(np.complex64).reshape(F, B)
        finally:
            mem.free(*ins, lm, ph, w, rec, X, cov, clm, cph, yb)
        res = []
        for i in range(n):
            a, b, T = foff[i], foff[i + 1], foff[i + 1] - foff[i]
            d = {"logmag": lm_h[a:b], "phase": ph_h[a:b], "w": w_h[i], "record": mvdr_mod.record(rec_h[i])}
            if stages:
                ch = lambda r: r[C * a:C * b].reshape(C, T, B)
                d.update(y=y_h[a:b], X=ch(X_h), chan_logmag=ch(clm_h), chan_phase=ch(cph_h),
                         phi_s=np.ascontiguousarray(cov_h[i, 0].transpose(2, 0, 1)), phi_n=np.ascontiguousarray(cov_h[i, 1].transpose(2, 0, 1)))
            res.append(d)
        return res

    def enhance_array(self, mixes, ctx_a, ctx_b, ref=0, mask_from="mean", post="none", loading=mvdr_mod.LOADING,
                      lookahead=spec.LOOKAHEAD, phase_iters=0, phase_alpha=0.0, taps=False, want_mixed=False):
        """Multi-channel clips through the network and an MVDR beamformer, on the device throughout.  mixes: a list of
        [n_i, C] float32 arrays, normalised and trimmed to whole frames as enhance takes its mixtures; ctx_a, ctx_b: the
        conditioning recordings, as for enhance.  The existing path runs on the mean of the channels (mask_from="mean":
        nhans_channel_mean, the signal enhance is given today, bit for bit) or on channel mask_from=j; nhans_mask_net's
        logits are the log-gain whose mask picks the covariances (nhans_mvdr, NHANS_MVDR_LOGGAIN, reference channel ref).
        post: what follows the beamformer -- "none": its rows go to nhans_istft; "mask": the same log-gain is added to them
        (in the filter's launch); "net": a second nhans_mask_net pass on them with the same embeddings.  phase_iters,
        phase_alpha: nhans_phase_refine on the final rows from the beamformed phase.  lookahead as in enhance; a saturated
        f16x3 batch is redone in f32 as everywhere.
        -> dict: "denoised_wav", one float32 array of (T_i - 1) 160 + 400 samples per clip; "records", one dict by
        mvdr.FIELDS per clip; want_mixed=True: plus "mixed_wav", the transform round trip of the signal the mask came from
        (enhance's mixed_wav of that signal); taps=True: plus "logits", "bf_logmag", "bf_phase", "logmag" and "phase" (the rows that went
        to nhans_istft), float32 [T_i, 201] per clip."""
        if post not in ("none", "mask", "net"):
            raise ValueError("enhance_array: post is 'none', 'mask' or 'net', not %r" % (post,))
        if phase_iters and not 0 < int(phase_iters) <= hip.PHASE_MAX_ITERS:
            raise ValueError("phase_iters 0 ... %d, not %r" % (hip.PHASE_MAX_ITERS, phase_iters))
        xs, C, pf, off, foff = self._array_clips("enhance_array", mixes)
        n, F, B = len(xs), foff[-1], spec.BINS
        if not (len(ctx_a) == len(ctx_b) == n):
            raise ValueError("enhance_array: one (a, b) pair of conditioning recordings per clip")
        if not isinstance(mask_from, str):
            try:
                mask_from = operator.index(mask_from)
            except TypeError:
                mask_from = None
        if mask_from != "mean" and not (isinstance(mask_from, int) and 0 <= mask_from < C):
            raise ValueError("enhance_array: mask_from is 'mean' or a channel 0 ... %d" % (C - 1))
        if not 0 <= int(ref) < C:
            raise ValueError("enhance_array: ref 0 ... %d, not %r" % (C - 1, ref))
        lib, mem = self.lib, Mem(self)
        (af, aoff), (bf, boff) = flat(ctx_a), flat(ctx_b)
        ooff = offsets((foff[i + 1] - foff[i] - 1) * spec.HOP + spec.WIN for i in range(n))
        ins = [mem.up(pf), mem.up(af), mem.up(bf)]
        mono = mem.empty(off[-1])
        names = ("lm", "ph", "logits", "den", "blm", "bph", "den2", "rph")
        r = {k: mem.empty(F * B) for k in names}
        ctx_lm, emb = mem.empty(2 * n * spec.NOISE_WIN * B), mem.empty(2 * n * spec.EMB)
        wav, rec = mem.empty(ooff[-1]), mem.empty(n * hip.MVDR_FIELDS, np.float64)
        mixed_wav = mem.empty(ooff[-1]) if want_mixed else None

        def at(buf, floats):
            return ctypes.c_void_p(mem.p(buf).value + 4 * floats)

        def run():
            c, h, s = hip.check, self.handle, mem.stream()
            fo = hip.i64_array(foff)
            for i in range(n):          # the signal the mask comes from: the channels' mean, or one channel (a mean of one)
                ni = off[i + 1] - off[i]
                src, k = (at(ins[0], C * off[i]), C) if mask_from == "mean" else (at(ins[0], C * off[i] + mask_from * ni), 1)
                c(lib.nhans_channel_mean(h, src, k, ni, at(mono, off[i]), s))
            c(lib.nhans_stft_features(h, mem.p(mono), hip.i64_array(off), n, 0, mem.p(r["lm"]), mem.p(r["ph"]), s))
            c(lib.nhans_stft_features(h, mem.p(ins[1]), hip.i64_array(aoff), n, spec.NOISE_WIN, mem.p(ctx_lm), None, s))
            c(lib.nhans_stft_features(h, mem.p(ins[2]), hip.i64_array(boff), n, spec.NOISE_WIN, at(ctx_lm, n * spec.NOISE_WIN * B), None, s))
            c(lib.nhans_embed(h, mem.p(ctx_lm), 2 * n, mem.p(emb), s))
            c(lib.nhans_mask_net(h, mem.p(r["lm"]), fo, n, mem.p(emb), at(emb, n * spec.EMB), mem.p(r["logits"]), mem.p(r["den"]), s))
            c(lib.nhans_mvdr(h, mem.p(ins[0]), hip.i64_array(off), n, C, mem.p(r["logits"]), int(ref), float(loading), hip.MVDR_LOGGAIN,
                             mem.p(r["logits"]) if post == "mask" else None, mem.p(r["blm"]), mem.p(r["bph"]), None, mem.p(rec), s))
            out_lm = r["blm"]
            if post == "net":
                c(lib.nhans_mask_net(h, mem.p(r["blm"]), fo, n, mem.p(emb), at(emb, n * spec.EMB), None, mem.p(r["den2"]), s))
                out_lm = r["den2"]
            out_ph = r["bph"]
            if phase_iters:
                c(lib.nhans_phase_refine(h, mem.p(out_lm), mem.p(r["bph"]), fo, n, int(phase_iters), float(phase_alpha), mem.p(r["rph"]),
                                         None, s))
                out_ph = r["rph"]
            c(lib.nhans_istft(h, mem.p(out_lm), mem.p(out_ph), fo, n, hip.i64_array(ooff), mem.p(wav), s))
            if want_mixed:
                c(lib.nhans_istft(h, mem.p(r["lm"]), mem.p(r["ph"]), fo, n, hip.i64_array(ooff), mem.p(mixed_wav), s))
            return out_lm, out_ph

        try:
            out_lm, out_ph = self._with_lookahead(lookahead, lambda: redo_saturated_in_f32(self, run))   # (take_status waits)
            g = lambda buf, cnt, dt=np.float32: np.array(mem.down(buf, cnt, dt), dtype=dt)
            wav_h = g(wav, ooff[-1])
            mixed_h = g(mixed_wav, ooff[-1]) if want_mixed else None
            rec_h = g(rec, n * hip.MVDR_FIELDS, np.float64).reshape(n, hip.MVDR_FIELDS)
            tap = {}
            if taps:
                tap = {k: g(b, F * B).reshape(F, B) for k, b in (("logits", r["logits"]), ("bf_logmag", r["blm"]), ("bf_phase", r["bph"]),
                                                               ("logmag", out_lm), ("phase", out_ph))}
        finally:
            mem.free(*ins, mono, *r.values(), ctx_lm, emb, wav, rec, mixed_wav)
        res = {"denoised_wav": [wav_h[ooff[i]:ooff[i + 1]] for i in range(n)], "records": [mvdr_mod.record(v) for v in rec_h]}
        if want_mixed:
            res["mixed_wav"] = [mixed_h[ooff[i]:ooff[i + 1]] for i in range(n)]
        for k, v in tap.items():
            res[k] = [v[foff[i]:foff[i + 1]] for i in range(n)]
        return res

    def _records_call(self, signals, nrec, nextra, call):
        """What the calls that return records share: the flat float32 `signals` uploaded as one buffer, one float64 output
        of nrec doubles of records and nextra of the optional output after them (None: not asked for), call(at, out, extra,
        stream) -> status -- at(k): where signal k begins on the device, out: the records, extra: the optional output or
        None --, the wait, and all nrec + nextra doubles downloaded; both buffers are freed whatever happened."""
        mem, nall = Mem(self), nrec + (nextra or 0)
        base = offsets(len(x) for x in signals)
        buf = mem.up(np.ascontiguousarray(np.concatenate(signals)))
        out = mem.empty(nall, np.float64)
        try:
            at = lambda k: ctypes.c_void_p(mem.p(buf).value + 4 * base[k])
            extra = None if nextra is None else ctypes.c_void_p(mem.p(out).value + 8 * nrec)
            hip.check(call(at, mem.p(out), extra, mem.stream()))
            self._sync()
            return np.array(mem.down(out, nall, np.float64), dtype=np.float64)
        finally:
            mem.free(buf, out)

    def _sync(self):
        """Waits for the work issued on this context's stream (the null stream's copies wait by themselves)."""


def quality_bands_arg(bands):
    """bands (None, or a [K <= 32, 257] matrix) -> (the host pointer nhans_quality takes, K)"""
    if bands is None:
        return None, 0
    W = np.ascontiguousarray(bands, dtype=np.float64)
    if W.ndim != 2 or W.shape[1] != hip.QUALITY_BINS:
        raise ValueError("quality: bands is a [K, %d] matrix" % hip.QUALITY_BINS)
    return W.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(W.shape[0])


def redo_saturated_in_f32(eng, run, undo=None):
    """run() -- the launches of one batch or push -- and its result; where they saturated the f16x3 path, run() again on
    the exact f32 path.  The split-f16 layout holds |activation * 2^-e| < 65504 and such work is further from the
    calibration than the 2^8 of headroom: undo() takes it back (a push: the rewind), then the same library does it in
    f32 MFMA mode (no CPU involved) with the tensors' maxima recorded, and the exponents are raised so that the work
    after it fits."""
    res = run()
    if not (eng.take_status() & hip.STATUS_SATURATED and eng.precision == "f16x3"):
        return res
    warnings.warn("N-HANS f16x3 path: an activation left the f16 range; batch recomputed in f32 MFMA mode "
                  "and the activation exponents raised")
    if undo is not None:
        undo()
    eng.set_option("calibrate", 1)
    try:
        eng.set_precision("f32")
        res = run()
        eng.take_status()
    except BaseException:
        # close the bracket FIRST (3 = keep the exponents, learn nothing) -- an open bracket keeps recording maxima on
        # every later call --, then put the precision back; neither may mask the original error
        try:
            eng.set_option("calibrate", 3)
        finally:
            eng.set_precision("f16x3")
        raise
    try:
        # (raise-only; maxima that are not finite -- the flag is also raised by a NaN / Inf INPUT -- are skipped)
        eng.set_option("calibrate", 2)
    except hip.NhansError as err:          # the f32 result stands whatever the exponent update says
        warnings.warn("N-HANS: activation exponents not updated after the f32 rerun: %s" % err)
    finally:
        eng.set_precision("f16x3")
    return res


class Mem:
    """Device memory and stream of either engine: the package's one branch between torch and hiprt.  A buffer of 0
    elements is one allocated element, so that its pointer is never null."""

    def __init__(self, engine):
        self.eng = engine
        self.torch = engine.torch_memory

    def stream(self):
        return self.eng._stream()

    def up(self, arr):
        """contiguous numpy array -> device copy"""
        if not self.torch:
            return hiprt.DevBuf.from_array(arr)
        if not arr.size:
            return self.empty(0, arr.dtype)
        import torch
        return torch.from_numpy(arr).to(self.eng.device)

    def up_f32(self, x):
        """A host array -- or, over torch memory, a tensor -- as (flat float32 device buffer, its elements, whether the
        buffer was allocated here and is the caller's to free)."""
        if self.torch and hasattr(x, "data_ptr"):
            import torch
            t = x.detach().to(device=self.eng.device, dtype=torch.float32).contiguous().reshape(-1)
            return t, t.numel(), False
        a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        return self.up(a), a.size, True

    def empty(self, n, dtype=np.float32):
        if self.torch:
            import torch
            return torch.empty(max(n, 1), dtype=getattr(torch, np.dtype(dtype).name), device=self.eng.device)
        return hiprt.DevBuf(np.dtype(dtype).itemsize * max(n, 1))

    def p(self, buf):
        if buf is None:
            return None
        return hip.ptr(buf) if self.torch else buf.ptr

    def down(self, buf, n, dtype=np.float32):
        if self.torch:
            return buf[:n].cpu().numpy()
        return buf.to_array(np.empty(n, dtype))

    def free(self, *bufs):
        if not self.torch:
            for b in bufs:
                if b is not None:
                    b.free()


def offsets(counts):
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


def flat(arrays, dtype=np.float32):
    """1-D arrays -> (one contiguous array of dtype holding them one after the other, offsets)."""
    off = offsets(len(a) for a in arrays)
    out = np.concatenate([np.asarray(a, dtype=dtype) for a in arrays]) if len(arrays) else np.zeros(0, dtype)
    return np.ascontiguousarray(out, dtype=dtype), off


def mix_job_arrays(jobs, speech_off):
    """jobs (speech index, keep index or -1, drop index, snr_keep_db, snr_drop_db) -> (the five host arrays nhans_mix
    takes, the output offsets: room for each job's speech length; an index out of range is the library's to refuse)."""
    nj, ns = len(jobs), len(speech_off) - 1
    si, ki, di = [(ctypes.c_int * nj)(*[int(j[k]) for j in jobs]) for k in range(3)]
    sk, sd = [(ctypes.c_double * nj)(*[float(j[k] or 0) for j in jobs]) for k in (3, 4)]     # (None: no keep noise, no SNR)
    off = offsets(speech_off[i + 1] - speech_off[i] if 0 <= i < ns else 0 for i in si)
    return (si, ki, di, sk, sd), off


def bss_call(lib, handle, est_p, est_off, src_ps, src_offs, n, filt_len, out_p, filters_p, stream):
    """nhans_bss_eval with its two host tables built from J device pointers and J offset lists -> the call's return code"""
    J = len(src_ps)
    ptrs = (ctypes.c_void_p * J)(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in src_ps])
    offs = [hip.i64_array(o) for o in src_offs]
    i64p = ctypes.POINTER(ctypes.c_int64)
    tab = (i64p * J)(*[ctypes.cast(o, i64p) for o in offs])
    return lib.nhans_bss_eval(handle, est_p, hip.i64_array(est_off), ptrs, tab, J, n, int(filt_len), out_p, filters_p, stream)


def end_flags(end, n):
    """end[i]: stream i ends after this push -> the int array the push entry points take (None: no stream ends)."""
    return (ctypes.c_int * n)(*[int(bool(e)) for e in end]) if end is not None else None
