// nhans_quality, nhans_quality_lpc, nhans_quality_tables (include/nhans_hip.h): the run table and the launches of
// quality.hip.  What the calls refuse needs no device and is refused before the context is looked at.
//   Workspace.  The run table, the window and twiddle table, the band matrix with its rows' spans and, where the caller does not take the
// per-frame values, three doubles a frame for them: 24 bytes a frame, 32 KB for a clip of 10 s.
#include "host_internal.h"

namespace {

// the checks the two calls share and the run table; *frames, *lt, *bt: the totals
int quality_runs(const std::string& fn, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips,
                 const void* out, std::vector<QualityRun>* runs, long long* frames, long long* lt, long long* bt) {
    *frames = *lt = *bt = 0;
    const int rc = pair_clips(fn, "score", est, eoff, tgt, toff, nclips, out, [&](int i, const float* e, const float* t, int64_t ne, int64_t nt) {
        const int64_t n = std::min(ne, nt);
        if (n > 0 && (!e || !t)) return null_clip(fn, i, n);
        if (n > kMaxResampleClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(n) + " samples (0 ... 2^31 - 1)");
        const long long m = quality_frames(n);
        runs->push_back({n > 0 ? e : nullptr, n > 0 ? t : nullptr, (long long)n, m, *frames, *lt, *bt});
        *frames += m;
        *lt += (m + kQualityLpcTile - 1) / kQualityLpcTile;
        *bt += (m + kQualityBandTile - 1) / kQualityBandTile;
        return NHANS_OK;
    });
    if (rc) return rc;
    if (*lt > 0x7fffffffLL || *bt > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many samples for one call (split it)");
    return NHANS_OK;
}

// per frame: 34 chains of about 472 steps, three operations a step; the recursions, forms and cepstra about 3,000 more
double lpc_flops(double F) { return F * (34.0 * 472.0 * 3.0 + 3000.0); }

}  // namespace

extern "C" {

int nhans_quality_tables(double* window_out, double* bands_out) {
    if (window_out) {
        std::vector<double> tab(kQualityTable);
        quality_table(tab.data());
        std::copy(tab.begin(), tab.begin() + kQualityFrame, window_out);
    }
    if (bands_out) quality_default_bands(bands_out);
    return NHANS_OK;
}

int nhans_quality(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips,
                  const double* bands, int nbands, double* out, double* frames_out, void* stream) {
    const std::string fn = "nhans_quality";
    if (bands) {
        if (nbands < 1 || nbands > kQualityMaxBands)
            return fail(NHANS_EINVAL, fn + ": " + std::to_string(nbands) + " bands (1 ... " + std::to_string(kQualityMaxBands) + ")");
        for (int j = 0; j < nbands; ++j)
            for (int k = 0; k < kQualityBins; ++k) {
                const double v = bands[(size_t)j * kQualityBins + k];
                if (!(v >= 0.0) || !(v <= std::numeric_limits<double>::max()))
                    return fail(NHANS_EINVAL, fn + ": band weight [" + std::to_string(j) + ", " + std::to_string(k) + "] is negative or not finite");
            }
    }
    std::vector<QualityRun> runs;
    long long frames = 0, lt = 0, bt = 0;
    int rc = quality_runs(fn, est, eoff, tgt, toff, nclips, out, &runs, &frames, &lt, &bt); if (rc) return rc;
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nclips == 0) return NHANS_OK;
        const int K = bands ? nbands : kQualityBands;
        WsPlan p;
        QualityRun* runs_dev; double *tab, *W, *vals; int* span_dev;
        p.add(&runs_dev, runs.size());
        p.add(&tab, kQualityTable);
        p.add(&W, (size_t)K * kQualityBins);
        p.add(&span_dev, (size_t)2 * K);
        p.add(&vals, frames_out ? 0 : (size_t)frames * 3);
        rc = ws_commit(c, p); if (rc) return rc;
        if (frames_out) vals = frames_out;
        rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
        std::vector<double> table(kQualityTable), wdef;
        quality_table(table.data());
        rc = h2d(c, tab, table, s); if (rc) return rc;
        if (!bands) {
            wdef.resize((size_t)kQualityBands * kQualityBins);
            quality_default_bands(wdef.data());
        }
        const double* wsrc = bands ? bands : wdef.data();
        rc = h2d(c, W, wsrc, (size_t)K * kQualityBins * sizeof(double), s); if (rc) return rc;
        // a row's chain runs from its first non-zero weight to its last: the zero weights outside add exact zeros
        std::vector<int> span((size_t)2 * K, 0);
        double terms = 0.0;
        for (int j = 0; j < K; ++j) {
            int lo = kQualityBins, hi = 0;
            for (int k = 0; k < kQualityBins; ++k)
                if (wsrc[(size_t)j * kQualityBins + k] != 0.0) { lo = std::min(lo, k); hi = k + 1; }
            if (hi > 0) { span[2 * j] = lo; span[2 * j + 1] = hi; terms += hi - lo; }
        }
        rc = h2d(c, span_dev, span, s); if (rc) return rc;
        const double F = (double)frames, C = (double)nclips;
        {   // a workgroup stages its tile's span of both signals once: 120 new samples a frame and signal, 480 at a tile's head
            Prof pr(c, s, "quality_lpc");
            launch_quality_lpc("quality_lpc", runs_dev, nclips, lt, tab, vals, nullptr, s);
            pr.done(lpc_flops(F), 2.0 * 4.0 * (kQualityHop * F + 360.0 * (double)lt) + 16.0 * F);
        }
        {   // per frame and signal: 480 products, 5 N log2 N of the transform, 4 a bin for the magnitude, 2 per band term worked
            Prof pr(c, s, "quality_bands");
            launch_quality_bands("quality_bands", runs_dev, nclips, bt, tab, W, span_dev, K, vals, s);
            pr.done(2.0 * F * (kQualityFrame + 5.0 * kQualityFft * 9.0 + 4.0 * kQualityBins + 2.0 * terms),
                    F * (2.0 * 4.0 * kQualityFrame + 8.0));
        }
        {   // per frame: three means, two selects of eight passes, two trimmed sums
            Prof pr(c, s, "quality_finish");
            launch_quality_finish("quality_finish", runs_dev, nclips, vals, out, s);
            pr.done(5.0 * F, 8.0 * F * (3.0 + 16.0 + 2.0) + 8.0 * kQualityFields * C);
        }
        return NHANS_OK;
    });
}

int nhans_quality_lpc(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips,
                      double* lpc_out, void* stream) {
    const std::string fn = "nhans_quality_lpc";
    std::vector<QualityRun> runs;
    long long frames = 0, lt = 0, bt = 0;
    int rc = quality_runs(fn, est, eoff, tgt, toff, nclips, lpc_out, &runs, &frames, &lt, &bt); if (rc) return rc;
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nclips == 0) return NHANS_OK;
        WsPlan p;
        QualityRun* runs_dev; double *tab, *vals;
        p.add(&runs_dev, runs.size());
        p.add(&tab, kQualityTable);
        p.add(&vals, (size_t)frames * 3);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
        std::vector<double> table(kQualityTable);
        quality_table(table.data());
        rc = h2d(c, tab, table, s); if (rc) return rc;
        {
            Prof pr(c, s, "quality_lpc");
            launch_quality_lpc("quality_lpc", runs_dev, nclips, lt, tab, vals, lpc_out, s);
            pr.done(lpc_flops((double)frames), 2.0 * 4.0 * (kQualityHop * (double)frames + 360.0 * (double)lt) + 8.0 * (2.0 + kQualityLpcFields) * (double)frames);
        }
        return NHANS_OK;
    });
}

}  // extern "C"
