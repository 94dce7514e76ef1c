// nhans_score_wave / nhans_score_rows (include/nhans_hip.h): the run tables and launches of score.hip.  What the two calls
// refuse needs no device and is refused before the context is looked at.
#include "host_internal.h"

extern "C" {

int nhans_score_wave(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips,
                     double* out, double* frames_out, void* stream) {
    const std::string fn = "nhans_score_wave";
    std::vector<ScoreRun> runs;
    long long tiles = 0, segs = 0, frames = 0, samples = 0;
    int rc = pair_clips(fn, "score", est, eoff, tgt, toff, nclips, out, [&](int i, const float* e, const float* t, int64_t ne, int64_t nt) {
        const int64_t n = std::min(ne, nt);
        if (n > 0 && (!e || !t)) return null_clip(fn, i, n);
        const int64_t nf = nhans_num_frames(n);
        runs.push_back({n > 0 ? e : nullptr, n > 0 ? t : nullptr, (long long)n, tiles, segs, frames, (long long)nf});
        tiles += (n + kScoreTile - 1) / kScoreTile;
        segs += (n + kScoreSegment - 1) / kScoreSegment;
        frames += nf;
        samples += n;
        return NHANS_OK;
    });
    if (rc) return rc;
    if (tiles > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many samples for one call (split it)");
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nclips == 0) return NHANS_OK;
        WsPlan p;
        ScoreRun* runs_dev; double *part, *segp;
        p.add(&runs_dev, runs.size());
        p.add(&part, (size_t)tiles * 4);
        p.add(&segp, (size_t)segs * 2);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
        const double n = (double)samples, T = (double)tiles, S = (double)segs, F = (double)frames, C = (double)nclips;
        {   // per sample: a subtraction and four fused multiply-adds, and the tree
            Prof pr(c, s, "score_pass1");
            launch_score_tiles("score_pass1", 1, runs_dev, nclips, tiles, part, segp, nullptr, s);
            pr.done(10.0 * n, 8.0 * n + 32.0 * T + 16.0 * S);
        }
        {
            Prof pr(c, s, "score_finish");
            launch_score_finish("score_finish", runs_dev, nclips, part, segp, out, frames_out, s);
            pr.done(4.0 * T + 12.0 * F, 32.0 * T + 80.0 * F + (frames_out ? 8.0 * F : 0.0) + 8.0 * kScoreFields * C);
        }
        {
            Prof pr(c, s, "score_pass2");
            launch_score_tiles("score_pass2", 2, runs_dev, nclips, tiles, part, segp, out, s);
            pr.done(5.0 * n, 8.0 * n + 8.0 * T);
        }
        {
            Prof pr(c, s, "score_si_sdr");
            launch_score_sisdr("score_si_sdr", runs_dev, nclips, part, out, s);
            pr.done(T + 5.0 * C, 8.0 * T + 32.0 * C);
        }
        return NHANS_OK;
    });
}

int nhans_score_rows(nhans_ctx* c, const float* est, const float* tgt, const int64_t* foff, int nclips, double* out,
                     double* frames_out, void* stream) {
    const std::string fn = "nhans_score_rows";
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (nclips > 0 && (!foff || !out)) return fail(NHANS_EINVAL, fn + ": null offsets or null output with " + std::to_string(nclips) + " clips to score");
    int rc = offsets_check(fn, "frame", foff, nclips); if (rc) return rc;
    std::vector<ScoreRowRun> runs((size_t)nclips);
    long long tiles = 0, frames = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t nf = foff[i + 1] - foff[i];
        if (nf > 0 && (!est || !tgt))
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(nf) + " rows and a null buffer");
        runs[i] = {nf > 0 ? est + foff[i] * kBins : nullptr, nf > 0 ? tgt + foff[i] * kBins : nullptr, (long long)nf, tiles, frames};
        tiles += (nf + kScoreRowTile - 1) / kScoreRowTile;
        frames += nf;
    }
    if (tiles > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many rows for one call (split it)");
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (nclips == 0) return NHANS_OK;
        WsPlan p;
        ScoreRowRun* runs_dev; double* vals;
        p.add(&runs_dev, runs.size());
        p.add(&vals, (size_t)frames * 2);
        rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
        const double F = (double)frames, C = (double)nclips;
        {   // per bin: a subtraction, three products and two fused multiply-adds
            Prof pr(c, s, "score_rows");
            launch_score_rows("score_rows", runs_dev, nclips, tiles, vals, frames_out, s);
            pr.done(8.0 * kBins * F, (8.0 * kBins + 16.0 + (frames_out ? 16.0 : 0.0)) * F);
        }
        {
            Prof pr(c, s, "score_rows_finish");
            launch_score_rows_finish("score_rows_finish", runs_dev, nclips, vals, out, s);
            pr.done(2.0 * F, 16.0 * F + 8.0 * kScoreRowFields * C);
        }
        return NHANS_OK;
    });
}

}  // extern "C"
