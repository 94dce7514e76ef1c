// ---- mask-driven MVDR beamforming (include/nhans_hip.h: nhans_mvdr_*) ---------------------------------------------------
// The three stages (spectra, weights, filter), each a plan of its scratch and its launches, and the four entry points:
// one per stage and nhans_mvdr, which runs the three on one plan with X, the covariances and w in the workspace.
#include "host_internal.h"

namespace {

// what every call refuses before it looks at a buffer: the channel count, the reference channel, the loading, and in the
// clips' offsets (samples: sample offsets per channel, else frame offsets) a descent or a clip without a frame
int shape_check(const std::string& fn, int nclips, int C, int ref, double loading, const int64_t* off, bool samples) {
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (C < 1 || C > kMvdrMaxChannels)
        return fail(NHANS_EINVAL, fn + ": nchannels must be in [1, " + std::to_string(kMvdrMaxChannels) + "] (got " + std::to_string(C) + ")");
    if (ref < 0 || ref >= C) return fail(NHANS_EINVAL, fn + ": ref must be in [0, nchannels) (got " + std::to_string(ref) + ")");
    if (!(loading >= 0.0) || !(loading <= 1.0)) return fail(NHANS_EINVAL, fn + ": loading must be in [0, 1]");
    if (!off) return fail(NHANS_EINVAL, fn + ": null offsets");
    const int rc = offsets_check(fn, samples ? "sample" : "frame", off, nclips); if (rc) return rc;
    for (int i = 0; i < nclips; ++i) {
        const int64_t t = samples ? nhans_num_frames(off[i + 1] - off[i]) : off[i + 1] - off[i];
        if (t < 1) return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has no frame");
        if (t > kMaxFramesPerClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has more than " + std::to_string(kMaxFramesPerClip) + " frames");
    }
    return NHANS_OK;
}

std::vector<int64_t> frame_offsets(const int64_t* soff, int nclips) {
    std::vector<int64_t> foff(nclips + 1, 0);
    for (int i = 0; i < nclips; ++i) foff[i + 1] = foff[i] + nhans_num_frames(soff[i + 1] - soff[i]);
    return foff;
}

// ---- spectra: the channel-clips as the transform's clips
struct SpectraBufs {
    int64_t* tabs;      // sample offsets, then frame offsets, of the nclips * C channel-clips
    int* blocks;
    size_t nblocks;
};
void spectra_plan(WsPlan& p, const int64_t* soff, int nclips, int C, SpectraBufs* b) {
    b->nblocks = 0;
    for (int i = 0; i < nclips; ++i)
        b->nblocks += (size_t)C * (size_t)((nhans_num_frames(soff[i + 1] - soff[i]) + kStftFramesPerBlock - 1) / kStftFramesPerBlock);
    p.add(&b->tabs, 2 * ((size_t)nclips * C + 1));
    p.add(&b->blocks, 2 * b->nblocks);
}
int spectra_run(nhans_ctx* c, const float* planes, const int64_t* soff, int nclips, int C, float* X, float* logmag, float* phase,
                const SpectraBufs& b, hipStream_t s) {
    const size_t ncc = (size_t)nclips * C;
    std::vector<int64_t> so(ncc + 1), fo(ncc + 1);
    std::vector<int> bclip, bf0;
    int64_t f = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = soff[i + 1] - soff[i], t = nhans_num_frames(n);
        for (int ch = 0; ch < C; ++ch) {
            const size_t cc = (size_t)i * C + ch;
            so[cc] = C * soff[i] + ch * n;
            fo[cc] = f;
            f += t;
            for (int64_t f0 = 0; f0 < t; f0 += kStftFramesPerBlock) { bclip.push_back((int)cc); bf0.push_back((int)f0); }
        }
    }
    so[ncc] = C * soff[nclips];
    fo[ncc] = f;
    int rc = h2d(c, b.tabs, so, s); if (rc) return rc;
    rc = h2d(c, b.tabs + ncc + 1, fo, s); if (rc) return rc;
    rc = h2d(c, b.blocks, bclip, s); if (rc) return rc;
    rc = h2d(c, b.blocks + b.nblocks, bf0, s); if (rc) return rc;
    ClipTable t{b.tabs, b.tabs + ncc + 1, nullptr};
    Prof pr(c, s, "mvdr_spectra");
    launch_mvdr_spectra(planes, t, b.blocks, b.blocks + b.nblocks, (int)b.nblocks, c->net.tw400, c->net.window, X, logmag, phase, s);
    pr.done(0, (double)f * (kHop * 4 + (2 + (logmag ? 1 : 0) + (phase ? 1 : 0)) * kBins * 4));
    return NHANS_OK;
}

// ---- weights
struct WeightBufs {
    int64_t* foff_dev;
    double *phi, *eref;
};
void weights_plan(WsPlan& p, int nclips, int C, bool phi_in_ws, WeightBufs* b) {
    p.add(&b->foff_dev, (size_t)nclips + 1);
    p.add(&b->phi, phi_in_ws ? (size_t)nclips * 4 * C * C * kBins : 0);
    p.add(&b->eref, (size_t)nclips * kBins);
}
// (foff_dev is uploaded by the caller)
void weights_run(nhans_ctx* c, const float* X, const float* mask, const int64_t* foff, int nclips, int C, int ref, double loading,
                 int flags, double* phi, double* w_out, double* rec_out, const WeightBufs& b, hipStream_t s) {
    {
        Prof pr(c, s, "mvdr_cov");
        launch_mvdr_cov(X, mask, b.foff_dev, nclips, C, ref, flags, phi, b.eref, s);
        pr.done(0, (double)foff[nclips] * kBins * (8.0 * C + 4.0) + (double)nclips * kBins * (64.0 * C * C + 8.0));
    }
    Prof pr(c, s, "mvdr_solve");
    launch_mvdr_solve(phi, b.eref, b.foff_dev, nclips, C, ref, loading, w_out, rec_out, s);
    pr.done(0, (double)nclips * kBins * (64.0 * C * C + 8.0 + 16.0 * C));
}

// ---- filter
struct ApplyBufs {
    int64_t* foff_dev;
    int* blocks;
    size_t nblocks;
    double* eframe;
};
void apply_plan(WsPlan& p, const int64_t* foff, int nclips, bool own_foff, bool energy, ApplyBufs* b) {
    b->nblocks = 0;
    for (int i = 0; i < nclips; ++i) b->nblocks += (size_t)((foff[i + 1] - foff[i] + kMvdrRun - 1) / kMvdrRun);
    p.add(&b->foff_dev, own_foff ? (size_t)nclips + 1 : 0);
    p.add(&b->blocks, 2 * b->nblocks);
    p.add(&b->eframe, energy ? (size_t)foff[nclips] : 0);
}
int apply_run(nhans_ctx* c, const float* X, const double* w, const float* gain, const int64_t* foff, const int64_t* foff_dev, int nclips,
              int C, float* logmag, float* phase, float* y, double* rec, const ApplyBufs& b, hipStream_t s) {
    std::vector<int> bclip, bf0;
    for (int i = 0; i < nclips; ++i)
        for (int64_t f0 = 0; f0 < foff[i + 1] - foff[i]; f0 += kMvdrRun) { bclip.push_back(i); bf0.push_back((int)f0); }
    int rc = h2d(c, b.blocks, bclip, s); if (rc) return rc;
    rc = h2d(c, b.blocks + b.nblocks, bf0, s); if (rc) return rc;
    {
        Prof pr(c, s, "mvdr_apply");
        launch_mvdr_apply(X, w, gain, foff_dev, b.blocks, b.blocks + b.nblocks, (int)b.nblocks, C, logmag, phase, y,
                          rec ? b.eframe : nullptr, s);
        pr.done(0, (double)foff[nclips] * kBins * (8.0 * C + 8.0 + (gain ? 4.0 : 0.0) + (y ? 8.0 : 0.0)));
    }
    if (rec) {
        Prof pr(c, s, "mvdr_energy");
        launch_mvdr_energy(b.eframe, foff_dev, nclips, rec, s);
        pr.done(0, (double)foff[nclips] * 8.0);
    }
    return NHANS_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

int nhans_mvdr_spectra(nhans_ctx* c, const float* planes, const int64_t* soff, int nclips, int C, float* X, float* logmag, float* phase,
                       void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const std::string fn = "nhans_mvdr_spectra";
        int rc = shape_check(fn, nclips, C, 0, 0.0, soff, true); if (rc) return rc;
        if (nclips == 0) return (int)NHANS_OK;
        if (!planes || !X) return fail(NHANS_EINVAL, fn + ": null buffer");
        WsPlan p; SpectraBufs sb;
        spectra_plan(p, soff, nclips, C, &sb);
        rc = ws_commit(c, p); if (rc) return rc;
        return spectra_run(c, planes, soff, nclips, C, X, logmag, phase, sb, s);
    });
}

int nhans_mvdr_weights(nhans_ctx* c, const float* X, const float* mask, const int64_t* foff, int nclips, int C, int ref, double loading,
                       int flags, double* w_out, double* cov_out, double* rec_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const std::string fn = "nhans_mvdr_weights";
        int rc = shape_check(fn, nclips, C, ref, loading, foff, false); if (rc) return rc;
        if (flags & ~NHANS_MVDR_LOGGAIN) return fail(NHANS_EINVAL, fn + ": unknown flag bits");
        if (nclips == 0) return (int)NHANS_OK;
        if (!X || !mask || !w_out) return fail(NHANS_EINVAL, fn + ": null buffer");
        WsPlan p; WeightBufs wb;
        weights_plan(p, nclips, C, !cov_out, &wb);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, wb.foff_dev, foff, (size_t)(nclips + 1) * 8, s); if (rc) return rc;
        weights_run(c, X, mask, foff, nclips, C, ref, loading, flags, cov_out ? cov_out : wb.phi, w_out, rec_out, wb, s);
        return (int)NHANS_OK;
    });
}

int nhans_mvdr_apply(nhans_ctx* c, const float* X, const double* w, const float* gain, const int64_t* foff, int nclips, int C,
                     float* logmag, float* phase, float* y, double* rec, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const std::string fn = "nhans_mvdr_apply";
        int rc = shape_check(fn, nclips, C, 0, 0.0, foff, false); if (rc) return rc;
        if (nclips == 0) return (int)NHANS_OK;
        if (!X || !w || !logmag || !phase) return fail(NHANS_EINVAL, fn + ": null buffer");
        WsPlan p; ApplyBufs ab;
        apply_plan(p, foff, nclips, true, rec != nullptr, &ab);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, ab.foff_dev, foff, (size_t)(nclips + 1) * 8, s); if (rc) return rc;
        return apply_run(c, X, w, gain, foff, ab.foff_dev, nclips, C, logmag, phase, y, rec, ab, s);
    });
}

int nhans_mvdr(nhans_ctx* c, const float* planes, const int64_t* soff, int nclips, int C, const float* mask, int ref, double loading,
               int flags, const float* gain, float* logmag, float* phase, double* w_out, double* rec_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const std::string fn = "nhans_mvdr";
        int rc = shape_check(fn, nclips, C, ref, loading, soff, true); if (rc) return rc;
        if (flags & ~NHANS_MVDR_LOGGAIN) return fail(NHANS_EINVAL, fn + ": unknown flag bits");
        if (nclips == 0) return (int)NHANS_OK;
        if (!planes || !mask || !logmag || !phase) return fail(NHANS_EINVAL, fn + ": null buffer");
        const std::vector<int64_t> foff = frame_offsets(soff, nclips);
        WsPlan p; SpectraBufs sb; WeightBufs wb; ApplyBufs ab;
        float* X; double* w;
        spectra_plan(p, soff, nclips, C, &sb);
        weights_plan(p, nclips, C, true, &wb);
        apply_plan(p, foff.data(), nclips, false, rec_out != nullptr, &ab);
        p.add(&X, (size_t)2 * C * foff[nclips] * kBins);
        p.add(&w, w_out ? 0 : (size_t)nclips * kBins * C * 2);
        rc = ws_commit(c, p); if (rc) return rc;
        if (w_out) w = w_out;
        rc = spectra_run(c, planes, soff, nclips, C, X, nullptr, nullptr, sb, s); if (rc) return rc;
        rc = h2d(c, wb.foff_dev, foff, s); if (rc) return rc;
        weights_run(c, X, mask, foff.data(), nclips, C, ref, loading, flags, wb.phi, w, rec_out, wb, s);
        return apply_run(c, X, w, gain, foff.data(), wb.foff_dev, nclips, C, logmag, phase, nullptr, rec_out, ab, s);
    });
}

}  // extern "C"
