// nhans_stoi, nhans_stoi_resample, nhans_stoi_out_count (include/nhans_hip.h): the run table and launches of stoi.hip, and
// the 16 -> 10 kHz conversion on the rate-conversion stage of host_rate.hip.  What the calls refuse needs no device and is
// refused before the context is looked at.
#include "host_internal.h"

namespace {

int stoi_resample_body(nhans_ctx* c, const float* in, const int64_t* inoff, int nclips, float* out, const int64_t* outoff,
                       const ResampleFilter& f, hipStream_t s) {
    std::vector<ResampleRun> runs;
    size_t lds = 0;
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = inoff[i + 1] - inoff[i], no = resample_out_count(f, n);
        rs_add_runs(runs, &lds, f, reinterpret_cast<const char*>(in + inoff[i]), nullptr, nullptr,
                    reinterpret_cast<char*>(out + outoff[i]), 4, nullptr, 0, (int)n, 0, no);
        tin += n; tout += no;
    }
    if (runs.empty()) return NHANS_OK;
    const float* tab = nullptr;
    const int rc = rs_table(c, &f, &tab); if (rc) return rc;
    return rs_launch(c, "stoi_resample", runs, tab, f, {false, kResampleFloat32, 0, 0.f, 0.0}, lds, 4.0 * (double)tin, 4.0 * (double)tout,
                     tout, s);
}

}  // namespace

extern "C" {

int64_t nhans_stoi_out_count(int64_t n16) {
    if (n16 < 0) return fail(NHANS_EINVAL, "nhans_stoi_out_count: negative sample count");
    return resample_out_count(*resample_filter_stoi(), n16);
}

int nhans_stoi_resample(nhans_ctx* c, const float* in, const int64_t* inoff, int nclips, float* out, const int64_t* outoff,
                        void* stream) {
    const std::string fn = "nhans_stoi_resample";
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (nclips > 0 && (!inoff || !outoff)) return fail(NHANS_EINVAL, fn + ": null offsets with " + std::to_string(nclips) + " clips to convert");
    int rc = offsets_check(fn, "input", inoff, nclips); if (rc) return rc;
    rc = offsets_check(fn, "output", outoff, nclips); if (rc) return rc;
    const ResampleFilter& f = *resample_filter_stoi();
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = inoff[i + 1] - inoff[i];
        if (n > kMaxResampleClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(n) + " samples (0 ... 2^31 - 1)");
        const int64_t no = resample_out_count(f, n);
        if (outoff[i + 1] - outoff[i] < no)
            return fail(NHANS_EINVAL, fn + ": output room of clip " + std::to_string(i) + " is " + std::to_string(outoff[i + 1] - outoff[i]) +
                                      " samples, " + std::to_string(no) + " needed (nhans_stoi_out_count)");
        if (n > 0 && (!in || !out)) return null_clip(fn, i, n);
    }
    return ctx_call(c, stream, [&](hipStream_t s) { return stoi_resample_body(c, in, inoff, nclips, out, outoff, f, s); });
}

int nhans_stoi(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips, double* out,
               double* segments_out, void* stream) {
    const std::string fn = "nhans_stoi";
    std::vector<StoiRun> runs;
    long long frames = 0, rows = 0, segs = 0, pt = 0, bt = 0, st = 0;
    int rc = pair_clips(fn, "score", est, eoff, tgt, toff, nclips, out, [&](int i, const float* e, const float* t, int64_t ne, int64_t nt) {
        const int64_t n = std::min(ne, nt);
        if (n > 0 && (!e || !t)) return null_clip(fn, i, n);
        const long long m0 = stoi_frames(n);
        if (m0 > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has too many samples for one call (split it)");
        const long long nb = std::max(m0 - 1, 0LL), ns = std::max(m0 - kStoiSegment, 0LL);
        runs.push_back({n > 0 ? e : nullptr, n > 0 ? t : nullptr, (long long)n, m0, frames, rows, segs, pt, bt, st});
        frames += m0; rows += nb; segs += ns;
        pt += (m0 + kStoiPowerTile - 1) / kStoiPowerTile;
        bt += (nb + kStoiBandTile - 1) / kStoiBandTile;
        st += (ns + kStoiSegTile - 1) / kStoiSegTile;
        return NHANS_OK;
    });
    if (rc) return rc;
    if (pt > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many samples for one call (split it)");
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nclips == 0) return NHANS_OK;
        WsPlan p;
        StoiRun* runs_dev; double *tab, *power, *bands, *segv; int* kept; long long* nkept;
        p.add(&runs_dev, runs.size());
        p.add(&tab, kStoiTable);
        p.add(&power, (size_t)frames);
        p.add(&kept, (size_t)frames);
        p.add(&nkept, runs.size());
        p.add(&bands, (size_t)rows * 2 * kStoiBands);
        p.add(&segv, (size_t)segs * 2);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
        std::vector<double> table(kStoiTable);
        stoi_table(table.data());
        rc = h2d(c, tab, table, s); if (rc) return rc;
        const double F = (double)frames, R = (double)rows, S = (double)segs, C = (double)nclips;
        {   // per sample of a frame: a product and a fused multiply-add
            Prof pr(c, s, "stoi_power");
            launch_stoi_power("stoi_power", runs_dev, nclips, pt, tab, power, s);
            pr.done(3.0 * kStoiFrame * F, 4.0 * kStoiFrame * F + 8.0 * F);
        }
        {
            Prof pr(c, s, "stoi_keep");
            launch_stoi_keep("stoi_keep", runs_dev, nclips, power, kept, nkept, s);
            pr.done(F, 16.0 * F + 4.0 * F + 8.0 * C);
        }
        {   // per frame and signal: 4 operations a sample, 5 N log2 N of the transform, 3 a bin; what is silent is not computed
            Prof pr(c, s, "stoi_bands");
            launch_stoi_bands("stoi_bands", runs_dev, nclips, bt, tab, kept, nkept, bands, rows, s);
            pr.done(2.0 * R * (4.0 * kStoiFrame + 5.0 * kStoiFft * 9.0 + 3.0 * 212.0), 2.0 * R * (8.0 * kStoiFrame + 8.0 * kStoiBands));
        }
        {   // per segment: about 30 operations a value of either tensor
            Prof pr(c, s, "stoi_segments");
            launch_stoi_segments("stoi_segments", runs_dev, nclips, st, nkept, bands, rows, segv, segments_out, s);
            pr.done(S * 2.0 * kStoiBands * kStoiSegment * 30.0, S * (2.0 * 8.0 * kStoiBands * kStoiSegment + 16.0 + (segments_out ? 16.0 : 0.0)));
        }
        {
            Prof pr(c, s, "stoi_finish");
            launch_stoi_finish("stoi_finish", runs_dev, nclips, nkept, segv, out, s);
            pr.done(2.0 * S, 16.0 * S + 8.0 * kStoiFields * C);
        }
        return NHANS_OK;
    });
}

}  // extern "C"
