// ---- phase refinement (include/nhans_hip.h: nhans_phase_*) -------------------------------------------------------------
// The scratch of a refinement (phase_plan), the launches of N iterations (phase_refine_run: nhans_phase_refine here and
// enhance_clips_body, host_net.hip, both go through it) and the two entry points.
#include "host_internal.h"

namespace {

// what both calls refuse in their clips: offsets that descend, a clip without a frame or beyond the kernels' range
int clips_check(const std::string& fn, const int64_t* foff, int nclips) {
    const int rc = offsets_check(fn, "frame", foff, nclips); if (rc) return rc;
    for (int i = 0; i < nclips; ++i) {
        const int64_t t = foff[i + 1] - foff[i];
        if (t < 1) return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has no frame");
        if (t > kMaxFramesPerClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has more than " + std::to_string(kMaxFramesPerClip) + " frames");
    }
    return NHANS_OK;
}

size_t run_count(const int64_t* foff, int nclips) {
    size_t nb = 0;
    for (int i = 0; i < nclips; ++i) nb += (size_t)((foff[i + 1] - foff[i] + kPhaseRun - 1) / kPhaseRun);
    return nb;
}

// the frame offsets and the run table on the device
int tables_upload(nhans_ctx* c, const int64_t* foff, int nclips, const PhaseBufs& pb, hipStream_t s) {
    std::vector<int> bclip, bf0;
    for (int i = 0; i < nclips; ++i)
        for (int64_t f0 = 0; f0 < foff[i + 1] - foff[i]; f0 += kPhaseRun) { bclip.push_back(i); bf0.push_back((int)f0); }
    int rc = h2d(c, pb.foff_dev, foff, (size_t)(nclips + 1) * 8, s); if (rc) return rc;
    rc = h2d(c, pb.blocks, bclip, s); if (rc) return rc;
    return h2d(c, pb.blocks + pb.nblocks, bf0, s);
}

// one projection launch and, where asked, the clips' inconsistency into column col of inc_out [nclips][stride]
void project(nhans_ctx* c, const PhaseBufs& pb, int nclips, int64_t total, const float* t_in, const float* d_prev, float alpha, float* d_out,
             float* t_out, double* inc_out, int stride, int col, hipStream_t s) {
    {
        Prof pr(c, s, "phase_project");
        launch_phase_project(pb.A, t_in, pb.foff_dev, pb.blocks, pb.blocks + pb.nblocks, (int)pb.nblocks, c->net.tw400, c->net.window,
                             c->net.wsyn, d_prev, alpha, d_out, t_out, inc_out ? pb.num : nullptr, s);
        pr.done(0, (double)total * kBins * (4.0 + 8.0 * (1 + (d_prev ? 1 : 0) + (d_out ? 1 : 0) + (t_out ? 1 : 0))));
    }
    if (inc_out) {
        Prof pr(c, s, "phase_inc");
        launch_phase_inc(pb.num, pb.den, pb.foff_dev, nclips, inc_out, stride, col, s);
        pr.done(0, (double)total * 16.0);
    }
}

}  // namespace

void phase_plan(WsPlan& p, const int64_t* foff, int nclips, bool momentum, PhaseBufs* pb) {
    const size_t total = (size_t)foff[nclips];
    pb->nblocks = run_count(foff, nclips);
    p.add(&pb->A, total * kBins);
    p.add(&pb->t[0], 2 * total * kBins);
    p.add(&pb->t[1], 2 * total * kBins);
    p.add(&pb->d, momentum ? 2 * total * kBins : 0);
    p.add(&pb->num, total);
    p.add(&pb->den, total);
    p.add(&pb->foff_dev, (size_t)nclips + 1);
    p.add(&pb->blocks, 2 * pb->nblocks);
}

int phase_refine_run(nhans_ctx* c, const float* logmag, const float* phase_in, const int64_t* foff, int nclips, int iters, double alpha,
                     float* phase_out, double* inc_out, const PhaseBufs& pb, hipStream_t s) {
    const int64_t total = foff[nclips];
    const int rc = tables_upload(c, foff, nclips, pb, s); if (rc) return rc;
    {
        Prof pr(c, s, "phase_prepare");
        launch_phase_prepare(logmag, phase_in, total, pb.A, pb.t[0], pb.den, s);
        pr.done(0, (double)total * kBins * 20.0);
    }
    const bool momentum = alpha != 0.0;
    for (int n = 0; n < iters; ++n) {
        // t_{n+1} = d_n + alpha (d_n - d_{n-1}), d_{-1} := d_0; the d plane is kept (in place) only where a later step reads it
        project(c, pb, nclips, total, pb.t[n & 1], momentum && n > 0 ? pb.d : nullptr, (float)alpha,
                momentum && n + 1 < iters ? pb.d : nullptr, pb.t[(n + 1) & 1], inc_out, iters, n, s);
        if (launch_error_pending()) return NHANS_OK;        // (the Call reports it)
    }
    Prof pr(c, s, "phase_angle");
    launch_phase_angle(pb.t[iters & 1], total * kBins, phase_out, s);
    pr.done(0, (double)total * kBins * 12.0);
    return NHANS_OK;
}

// ================================================================================================
extern "C" {

int nhans_phase_set_alpha(nhans_ctx* c, double alpha) {
    if (!c) return fail(NHANS_EINVAL, "nhans_phase_set_alpha: null argument");
    if (!(alpha >= 0.0) || !(alpha < 1.0)) return fail(NHANS_EINVAL, "nhans_phase_set_alpha: alpha must be in [0, 1)");
    c->phase_alpha = alpha;
    return NHANS_OK;
}

int nhans_phase_project(nhans_ctx* c, const float* logmag, const float* t, const int64_t* foff, int nclips, float* d_out,
                        double* inc_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const std::string fn = "nhans_phase_project";
        if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
        if (!foff) return fail(NHANS_EINVAL, fn + ": null offsets");
        int rc = clips_check(fn, foff, nclips); if (rc) return rc;
        if (nclips == 0) return (int)NHANS_OK;
        if (!logmag || !t || !d_out) return fail(NHANS_EINVAL, fn + ": null buffer");
        if (t == d_out) return fail(NHANS_EINVAL, fn + ": d_out_dev must not be t_dev (a run reads its neighbours' frames)");
        // (the plan of a refinement without its state planes: the caller's rows are the state)
        const int64_t total = foff[nclips];
        WsPlan p; PhaseBufs pb{};
        pb.nblocks = run_count(foff, nclips);
        p.add(&pb.A, (size_t)total * kBins);
        p.add(&pb.num, (size_t)total);
        p.add(&pb.den, (size_t)total);
        p.add(&pb.foff_dev, (size_t)nclips + 1);
        p.add(&pb.blocks, 2 * pb.nblocks);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = tables_upload(c, foff, nclips, pb, s); if (rc) return rc;
        {
            Prof pr(c, s, "phase_prepare");
            launch_phase_prepare(logmag, nullptr, total, pb.A, nullptr, pb.den, s);
            pr.done(0, (double)total * kBins * 8.0);
        }
        project(c, pb, nclips, total, t, nullptr, 0.f, d_out, nullptr, inc_out, 1, 0, s);
        return (int)NHANS_OK;
    });
}

int nhans_phase_refine(nhans_ctx* c, const float* logmag, const float* phase_in, const int64_t* foff, int nclips, int iters,
                       double alpha, float* phase_out, double* inc_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const std::string fn = "nhans_phase_refine";
        if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
        if (iters < 0 || iters > kPhaseMaxIters)
            return fail(NHANS_EINVAL, fn + ": iters must be in [0, " + std::to_string(kPhaseMaxIters) + "] (got " + std::to_string(iters) + ")");
        if (!(alpha >= 0.0) || !(alpha < 1.0)) return fail(NHANS_EINVAL, fn + ": alpha must be in [0, 1)");
        if (!foff) return fail(NHANS_EINVAL, fn + ": null offsets");
        int rc = clips_check(fn, foff, nclips); if (rc) return rc;
        if (nclips == 0) return (int)NHANS_OK;
        if (!logmag || !phase_in || !phase_out) return fail(NHANS_EINVAL, fn + ": null buffer");
        const int64_t total = foff[nclips];
        if (iters == 0) {       // the input phases, bit for bit
            if (phase_out != phase_in)
                HIP_TRY(hipMemcpyAsync(phase_out, phase_in, (size_t)total * kBins * 4, hipMemcpyDeviceToDevice, s));
            return (int)NHANS_OK;
        }
        WsPlan p; PhaseBufs pb;
        phase_plan(p, foff, nclips, alpha != 0.0, &pb);
        rc = ws_commit(c, p); if (rc) return rc;
        return phase_refine_run(c, logmag, phase_in, foff, nclips, iters, alpha, phase_out, inc_out, pb, s);
    });
}

}  // extern "C"
