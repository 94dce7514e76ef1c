// nhans_align, nhans_align_common, nhans_align_cut (include/nhans_hip.h): the run table and the launches of align.hip.
// What the calls refuse needs no device and is refused before the context is looked at.
//   Workspace.  The run table and, where the caller does not take the lag vectors, nclips (2 D + 1) doubles for them --
// nothing that grows with the number of sample tiles: a workgroup of align_corr carries its running sums itself.
#include "host_internal.h"

namespace {

int64_t align_common(int64_t ne, int64_t nt, int64_t d) {
    return std::max<int64_t>(0, std::min(ne - std::max<int64_t>(d, 0), nt - std::max<int64_t>(-d, 0)));
}

// 2 sum_d overlap(d): the algorithmic FLOP of one pair's lag vector
double align_flops(int64_t ne, int64_t nt, int D) {
    double f = 0.0;
    for (int64_t d = -D; d <= D; ++d) f += (double)std::max<int64_t>(0, std::min(nt, ne - d) - std::max<int64_t>(0, -d));
    return 2.0 * f;
}

}  // namespace

extern "C" {

int64_t nhans_align_common(int64_t ne, int64_t nt, int64_t delay) { return align_common(ne, nt, delay); }

int nhans_align(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips, int max_lag,
                double* out, double* corr_out, void* stream) {
    const std::string fn = "nhans_align";
    if (nclips >= 0 && (max_lag < 0 || max_lag > kAlignMaxLag))      // (a negative count is refused first, below)
        return fail(NHANS_EINVAL, fn + ": max_lag " + std::to_string(max_lag) + " (0 ... " + std::to_string(kAlignMaxLag) + ")");
    const int D = max_lag;
    std::vector<AlignRun> runs;
    int rc = pair_clips(fn, "align", est, eoff, tgt, toff, nclips, out, [&](int i, const float* e, const float* t, int64_t ne, int64_t nt) {
        if (ne > kMaxResampleClip || nt > kMaxResampleClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(std::max(ne, nt)) + " samples (0 ... 2^31 - 1)");
        if ((ne > 0 && !e) || (nt > 0 && !t)) return null_clip(fn, i, ne > 0 && !e ? ne : nt);
        runs.push_back({ne > 0 ? e : nullptr, nt > 0 ? t : nullptr, (long long)ne, (long long)nt});
        return NHANS_OK;
    });
    if (rc) return rc;
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nclips == 0) return NHANS_OK;
        const size_t nlags = (size_t)2 * D + 1;
        WsPlan p;
        AlignRun* runs_dev; double* corr;
        p.add(&runs_dev, runs.size());
        p.add(&corr, corr_out ? 0 : runs.size() * nlags);
        rc = ws_commit(c, p); if (rc) return rc;
        if (corr_out) corr = corr_out;
        rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
        const double C = (double)nclips, NL = (double)nlags;
        double flops = 0.0, samples = 0.0, staged = 0.0;
        if (c->profile) {
            const double nblk = (double)((nlags + kAlignLagBlock - 1) / kAlignLagBlock);
            for (const AlignRun& r : runs) {
                flops += align_flops(r.ne, r.nt, D);
                samples += (double)(r.ne + r.nt);
                staged += nblk * (double)((r.nt + kAlignTile - 1) / kAlignTile) * (2.0 * kAlignTile + kAlignLagBlock);
            }
        }
        {   // per lag and common sample: one fused multiply-add; a workgroup fetches a tile of t and the span of e it meets
            Prof pr(c, s, "align_corr");
            launch_align_corr("align_corr", runs_dev, nclips, D, corr, s);
            pr.done(flops, 4.0 * staged + 8.0 * C * NL);
        }
        {
            Prof pr(c, s, "align_pick");
            launch_align_pick("align_pick", runs_dev, nclips, D, corr, out, s);
            pr.done(2.0 * samples + C * NL, 4.0 * samples + 8.0 * C * NL + 8.0 * kAlignFields * C);
        }
        return NHANS_OK;
    });
}

int nhans_align_cut(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips,
                    const int64_t* delay, float* est_out, float* tgt_out, const int64_t* ooff, void* stream) {
    const std::string fn = "nhans_align_cut";
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (nclips > 0 && (!eoff || !toff || !delay || !ooff))
        return fail(NHANS_EINVAL, fn + ": null offsets or null delays with " + std::to_string(nclips) + " clips to cut");
    if ((est == nullptr) != (est_out == nullptr) || (tgt == nullptr) != (tgt_out == nullptr))
        return fail(NHANS_EINVAL, fn + ": a signal and its output are given together or left out together (one of a pair is null)");
    int rc = offsets_check(fn, "estimate", eoff, nclips); if (rc) return rc;
    rc = offsets_check(fn, "target", toff, nclips); if (rc) return rc;
    rc = offsets_check(fn, "output", ooff, nclips); if (rc) return rc;
    std::vector<AlignCopy> jobs;
    long long tiles = 0;
    double total = 0.0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t ne = eoff[i + 1] - eoff[i], nt = toff[i + 1] - toff[i], d = delay[i];
        if (d > ne || -d > nt)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + ": delay " + std::to_string(d) + " is more than the " +
                                      std::to_string(d > 0 ? ne : nt) + " samples of the " + (d > 0 ? "estimate" : "target") + " it shortens");
        const int64_t n = align_common(ne, nt, d);
        if (ooff[i + 1] - ooff[i] < n)
            return fail(NHANS_EINVAL, fn + ": output room of clip " + std::to_string(i) + " is " + std::to_string(ooff[i + 1] - ooff[i]) +
                                      " samples, " + std::to_string(n) + " needed (nhans_align_common)");
        if (n == 0) continue;
        for (int k = 0; k < 2; ++k) {
            const float* src = k ? tgt : est;
            if (!src) continue;
            jobs.push_back({src + (k ? toff[i] + std::max<int64_t>(-d, 0) : eoff[i] + std::max<int64_t>(d, 0)), (k ? tgt_out : est_out) + ooff[i],
                            (long long)n, tiles});
            tiles += (n + kAlignCutTile - 1) / kAlignCutTile;
            total += (double)n;
        }
    }
    if (tiles > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many samples for one call (split it)");
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (jobs.empty()) return NHANS_OK;
        AlignCopy* jobs_dev;
        rc = ws_upload(c, jobs, s, &jobs_dev); if (rc) return rc;
        {
            Prof pr(c, s, "align_cut");
            launch_align_cut("align_cut", jobs_dev, (int)jobs.size(), tiles, s);
            pr.done(0.0, 8.0 * total);
        }
        return NHANS_OK;
    });
}

}  // extern "C"
