// ---- sample-rate conversion and the file front end (include/nhans_hip.h: nhans_resample*, nhans_peak_normalise) --------
#include "host_internal.h"

namespace {

int rs_filter(const char* fn, int rate_in, int rate_out, const ResampleFilter** f) {
    *f = resample_filter(rate_in, rate_out);
    if (!*f)
        return fail(NHANS_EINVAL, std::string(fn) + ": " + std::to_string(rate_in) + " Hz -> " + std::to_string(rate_out) +
                                  " Hz is not supported (one side 16000 Hz, the other 8000, 11025, 12000, 16000, 22050, "
                                  "24000, 32000, 44100, 48000, 88200 or 96000 Hz)");
    return NHANS_OK;
}

}  // namespace

int rs_launch(nhans_ctx* c, const char* name, const std::vector<ResampleRun>& runs, const float* tab, const ResampleFilter& f,
              const RateIo& io, size_t lds, double in_bytes, double out_bytes, int64_t out_samples, hipStream_t s) {
    if (runs.empty()) return NHANS_OK;
    ResampleRun* runs_dev;
    const int rc = ws_upload(c, runs, s, &runs_dev); if (rc) return rc;
    Prof pr(c, s, name);
    launch_resample(name, runs_dev, (int)runs.size(), tab, f, io.from_mix, io.auto_wet, io.interleaved, io.pcm_format, io.quantise,
                    io.wet, io.factor, lds, s, io.highband);
    pr.done(2.0 * f.J * (double)out_samples, in_bytes + out_bytes + 4.0 * runs.size() * f.tab.size());
    return NHANS_OK;
}

int rs_table(nhans_ctx* c, const ResampleFilter* f, const float** tab) {
    float*& t = c->rs_tab[{f->rate_in, f->rate_out}];
    if (!t) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t), f->tab.size() * 4));
        const hipError_t e = hipMemcpy(t, f->tab.data(), f->tab.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(t); t = nullptr;
            return fail(NHANS_EHIP, std::string("hipMemcpy of the phase table: ") + hipGetErrorString(e));
        }
    }
    *tab = t;
    return NHANS_OK;
}

// THE run geometry: runs for outputs [m_begin, m_end) of one clip or stream whose n_new new samples are at src (mix: see
// ResampleRun) and follow absolute index k0, stored from dst on in elements of `elem` bytes; with hist_out also an
// empty run when there is no output, so that the carried samples follow every push that brought some
void rs_add_runs(std::vector<ResampleRun>& runs, size_t* lds, const ResampleFilter& f, const void* src, const float* mix,
                 const float* hist, char* dst, size_t elem, float* hist_out, int64_t k0, int n_new, int64_t m_begin, int64_t m_end) {
    bool first = true;
    for (int64_t m = m_begin; m < m_end || (first && hist_out); m += kResampleRun) {
        const int cnt = (int)std::max<int64_t>(0, std::min<int64_t>(kResampleRun, m_end - m));
        const int64_t t0 = m * f.M + f.half, q0 = t0 / f.L;
        const int p0 = (int)(t0 - q0 * f.L);
        runs.push_back({src, mix, hist, dst ? dst + (m - m_begin) * elem : nullptr, first ? hist_out : nullptr, (long long)k0,
                        (long long)(q0 - k0), p0, n_new, cnt});
        *lds = std::max(*lds, resample_run_lds_bytes(f, p0, cnt));
        first = false;
        if (cnt == 0) break;
    }
}

// One push through a stage, its arguments checked by the caller: the runs of every stream (stream i brings the samples
// [inoff[i], inoff[i + 1]) of `in` -- and of `mix`, where the kernel reads the mix --), ONE launch under `kernel`, then the
// commit.  Where the launch did not go out (a return code, or launch_error_pending()) nothing is committed.  gains
// (io.auto_wet): the table the runs of each stream read their hops' factors from.  il (io.interleaved): where stream i
// sits in the frames of the PCM side -- the counts stay those of inoff, and on that side the offsets are il's, in frames
// of il->ch elements, the run builder's step from one run's outputs to the next being one frame per output.  hb
// (io.highband): what the full-band sink adds to stream i's outputs, the k-th run of a stream beginning kResampleRun
// outputs after the one before.
int stage_push(nhans_ctx* c, RateStage& g, const char* kernel, const RateIo& io, const void* in, const float* mix,
               const int64_t* inoff, const int* end, void* out, const int64_t* outoff, int64_t* counts, hipStream_t s,
               const GainTab* gains, const Interleave* il, const HighBandIo* hb) {
    std::vector<ResampleRun> runs;
    std::vector<RateStage::Span> e(g.S);
    size_t lds = 0;
    int64_t tin = 0, tout = 0;
    const Interleave* il_src = io.from_mix ? nullptr : il;
    const Interleave* il_dst = io.from_mix ? il : nullptr;
    const size_t out_step = io.out_elem() * (il_dst ? il_dst->ch : 1);
    for (int i = 0; i < g.S; ++i) {
        const int64_t cnt = inoff[i + 1] - inoff[i];
        e[i] = g.plan(i, cnt, end && end[i]);
        const size_t first = runs.size();
        g.add_runs(runs, &lds, i, static_cast<const char*>(in) + (il_src ? il_src->base[i] : inoff[i]) * io.in_elem(),
                   mix ? mix + inoff[i] : nullptr,
                   out ? static_cast<char*>(out) + (il_dst ? il_dst->base[i] : outoff[i]) * io.out_elem() : nullptr, out_step, cnt, e[i]);
        for (size_t k = first; gains && k < runs.size(); ++k) {
            runs[k].wtab = gains->w + gains->off[i];
            runs[k].hop0 = g.st.N[i] / kHop;
        }
        for (size_t k = first; il && k < runs.size(); ++k) {
            if (il_src) { runs[k].src_ch = il->ch; runs[k].src_sum = il->n; }
            else { runs[k].dst_ch = il->ch; runs[k].dst_copies = il->n; }
        }
        for (size_t k = first; hb && k < runs.size(); ++k)
            highband_run(runs[k], hb->gain[i], hb->hold[i], hb->base[i], hb->n_old[i], hb->cnt[i],
                         static_cast<const char*>(hb->in) + hb->pos[i] * rs_elem(hb->fmt), hb->fmt, hb->ch, hb->sum, hb->denom,
                         e[i].Eo + (int64_t)(k - first) * kResampleRun);
        tin += cnt; tout += e[i].En - e[i].Eo;
    }
    const int rc = rs_launch(c, kernel, runs, g.tab, *g.f, io, lds, (double)tin * (io.in_elem() * (il_src ? il_src->n : 1) + (mix ? 4 : 0)),
                             (double)tout * (io.out_elem() * (il_dst ? il_dst->n : 1) + (hb ? 4 : 0)), tout, s);
    if (rc) return rc;
    if (launch_error_pending()) return NHANS_OK;
    for (int i = 0; i < g.S; ++i) {
        counts[i] = e[i].En - e[i].Eo;
        g.commit(i, inoff[i + 1] - inoff[i], end && end[i]);
    }
    return NHANS_OK;
}

struct nhans_resampler {
    nhans_ctx* c = nullptr;
    int device = 0, in_format = 0, flags = 0;
    double denom = 0.0;             // nhans_resampler_set_peak: peak + 1e-6; 0 = outputs as they are
    RateStage g;
    RateIo io() const { return {false, in_format, flags & NHANS_RESAMPLE_QUANTISE, 0.f, denom}; }
};

namespace {

int resample_body(nhans_ctx* c, const void* in, int fmt, const int64_t* inoff, int nclips, int rate_in, int rate_out,
                  int flags, float* out, const int64_t* outoff, hipStream_t s) {
    if (!inoff || !outoff || nclips < 0) return fail(NHANS_EINVAL, "nhans_resample: null argument");
    if (fmt != kResampleInt16 && fmt != kResampleFloat32) return fail(NHANS_EINVAL, "nhans_resample: in_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32");
    if (flags & ~NHANS_RESAMPLE_QUANTISE) return fail(NHANS_EINVAL, "nhans_resample: unknown flag");
    const ResampleFilter* f = nullptr;
    int rc = rs_filter("nhans_resample", rate_in, rate_out, &f); if (rc) return rc;
    std::vector<ResampleRun> runs;
    size_t lds = 0;
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = inoff[i + 1] - inoff[i];
        if (n < 0 || n > kMaxResampleClip)
            return fail(NHANS_EINVAL, "nhans_resample: clip " + std::to_string(i) + " has " + std::to_string(n) + " samples (0 ... 2^31 - 1)");
        const int64_t no = resample_out_count(*f, n);
        if (outoff[i + 1] - outoff[i] < no)
            return fail(NHANS_EINVAL, "nhans_resample: output room of clip " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " + std::to_string(no) +
                                      " needed (nhans_resample_out_count)");
        tin += n; tout += no;
    }
    if ((tin > 0 && !in) || (tout > 0 && !out)) return fail(NHANS_EINVAL, "nhans_resample: null buffer");
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = inoff[i + 1] - inoff[i];
        rs_add_runs(runs, &lds, *f, static_cast<const char*>(in) + inoff[i] * rs_elem(fmt), nullptr, nullptr,
                    reinterpret_cast<char*>(out + outoff[i]), 4, nullptr, 0, (int)n, 0, resample_out_count(*f, n));
    }
    if (runs.empty()) return NHANS_OK;
    const float* tab = nullptr;
    rc = rs_table(c, f, &tab); if (rc) return rc;
    return rs_launch(c, "resample", runs, tab, *f, {false, fmt, flags & NHANS_RESAMPLE_QUANTISE, 0.f, 0.0}, lds,
                     (double)tin * rs_elem(fmt), 4.0 * (double)tout, tout, s);
}

int peak_normalise_body(nhans_ctx* c, const float* in, const int64_t* off, int nclips, int flags, float* out, hipStream_t s) {
    if (!off || nclips < 0) return fail(NHANS_EINVAL, "nhans_peak_normalise: null argument");
    if (flags & ~NHANS_NORMALISE_WRAP_INT16) return fail(NHANS_EINVAL, "nhans_peak_normalise: unknown flag");
    std::vector<NormBlock> blocks;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = off[i + 1] - off[i];
        if (n < 0) return fail(NHANS_EINVAL, "nhans_peak_normalise: clip " + std::to_string(i) + " has a negative sample count");
        const int64_t nb = (n + kNormBlock - 1) / kNormBlock;
        if ((int64_t)blocks.size() + nb > (int64_t)1 << 30) return fail(NHANS_EINVAL, "nhans_peak_normalise: batch too large for one call");
        const int pb0 = (int)blocks.size();
        for (int64_t b = 0; b < nb; ++b)
            blocks.push_back({(long long)(off[i] + b * kNormBlock), (int)std::min<int64_t>(kNormBlock, n - b * kNormBlock), pb0, (int)nb});
    }
    if (blocks.empty()) return NHANS_OK;
    if (!in || !out) return fail(NHANS_EINVAL, "nhans_peak_normalise: null buffer");
    WsPlan p;
    NormBlock* bd; float* partial;
    p.add(&bd, blocks.size());
    p.add(&partial, blocks.size());
    int rc = ws_commit(c, p); if (rc) return rc;
    rc = h2d(c, bd, blocks, s); if (rc) return rc;
    const double n = (double)(off[nclips] - off[0]);
    { Prof pr(c, s, "peak_partial"); launch_peak_partial(in, bd, (int)blocks.size(), flags & NHANS_NORMALISE_WRAP_INT16, partial, s); pr.done(0, 4.0 * n); }
    if (launch_error_pending()) return NHANS_OK;
    { Prof pr(c, s, "peak_normalise"); launch_peak_normalise(in, bd, (int)blocks.size(), partial, out, s); pr.done(0, 8.0 * n); }
    return NHANS_OK;
}

int resampler_check_push(const nhans_resampler* o, const char* fn, int i, int64_t cnt, bool en) {
    return push_check(fn, "stream", i, cnt, en, o->g.st.ended[i], nullptr, kMaxResampleClip);
}

int resampler_push_body(nhans_resampler* o, const void* in, const int64_t* inoff, const int* end, float* out,
                        const int64_t* outoff, int64_t* counts, hipStream_t s) {
    if (!inoff || !outoff || !counts) return fail(NHANS_EINVAL, "nhans_resampler_push: null argument");
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < o->g.S; ++i) {
        const int64_t cnt = inoff[i + 1] - inoff[i];
        const bool en = end && end[i];
        const int rc = resampler_check_push(o, "nhans_resampler_push", i, cnt, en); if (rc) return rc;
        const RateStage::Span e = o->g.plan(i, cnt, en);
        if (outoff[i + 1] - outoff[i] < e.En - e.Eo)
            return fail(NHANS_EINVAL, "nhans_resampler_push: output room of stream " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " + std::to_string(e.En - e.Eo) +
                                      " needed (nhans_resampler_out_counts)");
        tin += cnt; tout += e.En - e.Eo;
    }
    if ((tin > 0 && !in) || (tout > 0 && !out)) return fail(NHANS_EINVAL, "nhans_resampler_push: null buffer");
    return stage_push(o->c, o->g, "resampler_push", o->io(), in, nullptr, inoff, end, out, outoff, counts, s);
}

}  // namespace

// ================================================================================================
extern "C" {

int64_t nhans_resample_out_count(int64_t n, int rate_in, int rate_out) {
    const ResampleFilter* f = nullptr;
    if (rs_filter("nhans_resample_out_count", rate_in, rate_out, &f)) return NHANS_EINVAL;
    if (n < 0) return fail(NHANS_EINVAL, "nhans_resample_out_count: negative sample count");
    return resample_out_count(*f, n);
}

int64_t nhans_resample_emitted(int64_t n, int ended, int rate_in, int rate_out) {
    const ResampleFilter* f = nullptr;
    if (rs_filter("nhans_resample_emitted", rate_in, rate_out, &f)) return NHANS_EINVAL;
    if (n < 0) return fail(NHANS_EINVAL, "nhans_resample_emitted: negative sample count");
    return resample_emitted(*f, n, ended != 0);
}

int nhans_resample_taps(int rate_in, int rate_out, double* out, int cap) {
    const ResampleFilter* f = nullptr;
    const int rc = rs_filter("nhans_resample_taps", rate_in, rate_out, &f); if (rc) return rc;
    const int n = (int)f->h.size();
    if (out) {
        if (cap < n) return fail(NHANS_EINVAL, "nhans_resample_taps: room for " + std::to_string(cap) + " taps, " + std::to_string(n) + " needed");
        std::memcpy(out, f->h.data(), (size_t)n * sizeof(double));
    }
    return n;
}

int nhans_resample(nhans_ctx* c, const void* in, int in_format, const int64_t* inoff, int nclips, int rate_in, int rate_out,
                   int flags, float* out, const int64_t* outoff, void* stream) {
    return ctx_call(c, stream,
                    [&](hipStream_t s) { return resample_body(c, in, in_format, inoff, nclips, rate_in, rate_out, flags, out, outoff, s); });
}

int nhans_peak_normalise(nhans_ctx* c, const float* in, const int64_t* off, int nclips, int flags, float* out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) { return peak_normalise_body(c, in, off, nclips, flags, out, s); });
}

int nhans_channel_mean(nhans_ctx* c, const float* in, int nchan, int64_t n, float* out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nchan < 1 || n < 0 || n >= ((int64_t)1 << 39)) return fail(NHANS_EINVAL, "nhans_channel_mean: nchannels must be >= 1 and 0 <= nsamples < 2^39");
        if (n > 0 && (!in || !out)) return fail(NHANS_EINVAL, "nhans_channel_mean: null buffer");
        Prof pr(c, s, "channel_mean");
        launch_channel_mean(in, nchan, n, out, s);
        pr.done(0, 4.0 * (double)n * (nchan + 1));
        return NHANS_OK;
    });
}

int nhans_resampler_open(nhans_ctx* c, int nstreams, int rate_in, int rate_out, int in_format, int flags, nhans_resampler** out) {
    if (!out) return fail(NHANS_EINVAL, "nhans_resampler_open: null argument");
    *out = nullptr;
    int rc = check_ctx(c); if (rc) return rc;
    if (nstreams < 1) return fail(NHANS_EINVAL, "nhans_resampler_open: nstreams must be >= 1");
    if (in_format != kResampleInt16 && in_format != kResampleFloat32)
        return fail(NHANS_EINVAL, "nhans_resampler_open: in_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32");
    if (flags & ~NHANS_RESAMPLE_QUANTISE) return fail(NHANS_EINVAL, "nhans_resampler_open: unknown flag");
    const ResampleFilter* f = nullptr;
    rc = rs_filter("nhans_resampler_open", rate_in, rate_out, &f); if (rc) return rc;
    nhans_resampler* o = new nhans_resampler();
    o->c = c; o->device = c->device; o->in_format = in_format; o->flags = flags;
    rc = o->g.alloc(c, "nhans_resampler_open", f, nstreams);
    if (rc) { delete o; return rc; }
    *out = o;
    return NHANS_OK;
}

int nhans_resampler_set_peak(nhans_resampler* o, double peak) {
    if (!o) return fail(NHANS_EINVAL, "nhans_resampler_set_peak: null object");
    if (!(peak >= 0.0) || !std::isfinite(peak)) return fail(NHANS_EINVAL, "nhans_resampler_set_peak: the peak must be finite and >= 0");
    o->denom = peak + 0.000001;
    return NHANS_OK;
}

int nhans_resampler_push(nhans_resampler* o, const void* in, const int64_t* inoff, const int* end, float* out,
                         const int64_t* outoff, int64_t* counts, void* stream) {
    return object_call(o, "nhans_resampler_push: null object", stream,
                       [&](hipStream_t s) { return resampler_push_body(o, in, inoff, end, out, outoff, counts, s); });
}

int nhans_resampler_out_counts(const nhans_resampler* o, const int64_t* in_counts, const int* end, int64_t* counts) {
    if (!o || !in_counts || !counts) return fail(NHANS_EINVAL, "nhans_resampler_out_counts: null argument");
    for (int i = 0; i < o->g.S; ++i) {
        const int rc = resampler_check_push(o, "nhans_resampler_out_counts", i, in_counts[i], end && end[i]); if (rc) return rc;
    }
    for (int i = 0; i < o->g.S; ++i) {
        const RateStage::Span e = o->g.plan(i, in_counts[i], end && end[i]);
        counts[i] = e.En - e.Eo;
    }
    return NHANS_OK;
}

int nhans_resampler_restart(nhans_resampler* o, int i) {
    if (!o) return fail(NHANS_EINVAL, "nhans_resampler_restart: null object");
    if (i < 0 || i >= o->g.S)
        return fail(NHANS_EINVAL, "nhans_resampler_restart: stream " + std::to_string(i) + " out of range (0 ... " + std::to_string(o->g.S - 1) + ")");
    o->g.restart(i);
    return NHANS_OK;
}

void nhans_resampler_close(nhans_resampler* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    o->g.release();
    delete o;
}

}  // extern "C"
