// nhans_drift_table, nhans_drift_segments, nhans_drift_range, nhans_drift_fit, nhans_drift_track, nhans_drift_warp
// (include/nhans_hip.h): the segment table, the line fit and the launches of drift.hip.  What the calls refuse needs no
// device and is refused before the context is looked at.  Compiled with contraction off: the fit and the centre lags are
// restated operation by operation in nhans_amd/score.py.
//   Workspace.  The segment or job table and, where the caller does not take the lag vectors, none for them: a workgroup of
// drift_track keeps its vector in LDS.  The interpolation table is designed and uploaded once per context (524,544 bytes).
#include "host_internal.h"

#pragma clang fp contract(off)

namespace {

// the table on the device: G then D
int drift_tab_dev(nhans_ctx* c, const double** tab) {
    if (!c->drift_tab) {
        std::vector<double> t((size_t)kDriftTableG + kDriftTableD);
        drift_table(t.data(), t.data() + kDriftTableG);
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->drift_tab), t.size() * 8));
        const hipError_t e = hipMemcpy(c->drift_tab, t.data(), t.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(c->drift_tab); c->drift_tab = nullptr;
            return fail(NHANS_EHIP, std::string("hipMemcpy of the drift table: ") + hipGetErrorString(e));
        }
    }
    *tab = c->drift_tab;
    return NHANS_OK;
}

std::string num(double v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

// what every call refuses of a line (a, b) of clip i
int line_check(const std::string& fn, int i, double a, double b) {
    if (!std::isfinite(a) || !std::isfinite(b))
        return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + ": the line (" + num(a) + ", " + num(b) + ") is not finite");
    if (std::fabs(b) > kDriftMaxSlope)
        return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + ": drift " + num(b) + " is outside -2^-10 ... 2^-10");
    if (std::fabs(a) > kDriftMaxDelay)
        return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + ": delay " + num(a) + " leaves the int32 range");
    return NHANS_OK;
}

// [u_lo, u_hi): the u of [0, nt) with 0 <= p(u) <= ne - 1; p is strictly increasing over the lines line_check admits
void drift_range(int64_t ne, int64_t nt, double a, double b, int64_t* u_lo, int64_t* u_hi) {
    *u_lo = *u_hi = 0;
    if (ne <= 0 || nt <= 0) return;
    const double top = (double)(ne - 1);
    int64_t lo = 0, hi = nt;                    // the first u with p(u) >= 0
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (drift_pos(a, b, (double)mid) >= 0.0) hi = mid; else lo = mid + 1;
    }
    const int64_t first = lo;
    hi = nt;                                    // the first u with p(u) > ne - 1
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (drift_pos(a, b, (double)mid) > top) hi = mid; else lo = mid + 1;
    }
    if (lo > first) { *u_lo = first; *u_hi = lo; }
}

struct Line { double a, b; bool ok; };

// the weighted least squares of tau on u over the segments of `use`, weights E_t, every sum ascending from +0.0
Line fit_line(const double* rec, const std::vector<int>& use) {
    double W = 0.0, su = 0.0, st = 0.0;
    for (int j : use) {
        const double* r = rec + (size_t)j * kDriftFields;
        W = W + r[3];
        su = su + r[3] * r[0];
        st = st + r[3] * r[1];
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (!(W > 0.0)) return {nan, nan, false};
    const double mu = su / W, mt = st / W;
    double Suu = 0.0, Sut = 0.0;
    for (int j : use) {
        const double* r = rec + (size_t)j * kDriftFields;
        const double du = r[0] - mu, dt = r[1] - mt, wdu = r[3] * du;
        Suu = Suu + wdu * du;
        Sut = Sut + wdu * dt;
    }
    if (!(Suu > 0.0)) return {nan, nan, false};
    const double b = Sut / Suu;
    return {mt - b * mu, b, true};
}

double residual(const double* r, const Line& f) { return r[1] - (f.a + f.b * r[0]); }

}  // namespace

extern "C" {

int nhans_drift_table(double* g_out, double* d_out) {
    drift_table(g_out, d_out);
    return NHANS_OK;
}

int64_t nhans_drift_segments(int64_t nt) { return drift_segments(nt); }

int nhans_drift_range(int64_t ne, int64_t nt, double a, double b, int64_t* u_lo, int64_t* u_hi) {
    const std::string fn = "nhans_drift_range";
    if (!u_lo || !u_hi) return fail(NHANS_EINVAL, fn + ": null output");
    if (ne < 0 || nt < 0 || ne > kMaxResampleClip || nt > kMaxResampleClip)
        return fail(NHANS_EINVAL, fn + ": " + std::to_string(ne) + " and " + std::to_string(nt) + " samples (0 ... 2^31 - 1)");
    const int rc = line_check(fn, 0, a, b); if (rc) return rc;
    drift_range(ne, nt, a, b, u_lo, u_hi);
    return NHANS_OK;
}

int nhans_drift_fit(const double* rec, int nseg, double rho_min, double trim, double* out) {
    const std::string fn = "nhans_drift_fit";
    if (nseg < 0) return fail(NHANS_EINVAL, fn + ": negative segment count");
    if (!out || (nseg > 0 && !rec)) return fail(NHANS_EINVAL, fn + ": null records or null output");
    if (!(rho_min == rho_min) || !(trim >= 0.0)) return fail(NHANS_EINVAL, fn + ": rho_min " + num(rho_min) + ", trim " + num(trim) + " (a number, trim >= 0)");
    std::vector<int> use;
    for (int j = 0; j < nseg; ++j) {
        const double* r = rec + (size_t)j * kDriftFields;
        if (r[6] == 0.0 && r[2] >= rho_min) use.push_back(j);
    }
    const double n_valid = (double)use.size();
    Line f = fit_line(rec, use);
    if (f.ok) {
        std::vector<int> kept;
        for (int j : use)
            if (std::fabs(residual(rec + (size_t)j * kDriftFields, f)) <= trim) kept.push_back(j);
        if (kept.size() != use.size()) {
            use.swap(kept);
            f = fit_line(rec, use);
        }
    }
    double rms = std::numeric_limits<double>::quiet_NaN();
    if (f.ok) {
        double W = 0.0, S = 0.0;
        for (int j : use) {
            const double* r = rec + (size_t)j * kDriftFields;
            const double e = residual(r, f), we = r[3] * e;
            W = W + r[3];
            S = S + we * e;
        }
        rms = std::sqrt(S / W);
    }
    out[0] = f.a; out[1] = f.b; out[2] = n_valid; out[3] = (double)use.size(); out[4] = rms;
    out[5] = f.ok && use.size() >= 3 && std::fabs(f.b) <= kDriftMaxSlope ? 1.0 : 0.0;
    return NHANS_OK;
}

int nhans_drift_track(nhans_ctx* c, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff, int nclips,
                      const double* ca, const double* cb, int radius, double* out, double* corr_out, void* stream) {
    const std::string fn = "nhans_drift_track";
    if (nclips >= 0 && (radius < 1 || radius > kDriftMaxR))         // (a negative count is refused first, below)
        return fail(NHANS_EINVAL, fn + ": radius " + std::to_string(radius) + " (1 ... " + std::to_string(kDriftMaxR) + ")");
    if (nclips > 0 && (!ca || !cb)) return fail(NHANS_EINVAL, fn + ": null centre lines with " + std::to_string(nclips) + " clips to track");
    const int R = radius;
    std::vector<DriftSeg> segs;
    int rc = pair_clips(fn, "track", est, eoff, tgt, toff, nclips, out, [&](int i, const float* e, const float* t, int64_t ne, int64_t nt) {
        if (ne > kMaxResampleClip || nt > kMaxResampleClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(std::max(ne, nt)) + " samples (0 ... 2^31 - 1)");
        if ((ne > 0 && !e) || (nt > 0 && !t)) return null_clip(fn, i, ne > 0 && !e ? ne : nt);
        const int rl = line_check(fn, i, ca[i], cb[i]); if (rl) return rl;
        const int64_t J = drift_segments(nt);
        for (int64_t j = 0; j < J; ++j) {
            const double zc = std::floor(std::fma(cb[i], (double)(j * kDriftHop) + 0.5 * (kDriftBlock - 1), ca[i]) + 0.5);
            if (std::fabs(zc) + R + kDriftT > 2147483647.0)
                return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + ": the lags around centre " + num(zc) + " of segment " +
                                          std::to_string(j) + " leave the int32 range");
            segs.push_back({ne > 0 ? e : nullptr, t + j * kDriftHop, (long long)ne, (long long)(j * kDriftHop), (int)zc, 0});
        }
        return NHANS_OK;
    });
    if (rc) return rc;
    if (segs.size() > 0x7fffffffu) return fail(NHANS_EINVAL, fn + ": too many segments for one call (split it)");
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (segs.empty()) return NHANS_OK;
        const double* tab;
        rc = drift_tab_dev(c, &tab); if (rc) return rc;
        DriftSeg* segs_dev;
        rc = ws_upload(c, segs, s, &segs_dev); if (rc) return rc;
        {   // per segment and lag 4,096 fused multiply-adds; a workgroup fetches its block of t and the span of e it meets
            const double S = (double)segs.size(), NL = 2.0 * (R + kDriftT) + 1.0;
            Prof pr(c, s, "drift_track");
            launch_drift_track("drift_track", segs_dev, (int)segs.size(), R, tab, out, corr_out, s);
            pr.done(2.0 * S * NL * kDriftBlock, S * (4.0 * (2.0 * kDriftBlock + NL) + 8.0 * kDriftFields + (corr_out ? 8.0 * NL : 0.0)));
        }
        return NHANS_OK;
    });
}

int nhans_drift_warp(nhans_ctx* c, const float* est, const int64_t* eoff, const int64_t* toff, int nclips, const double* a,
                     const double* b, float* out, const int64_t* ooff, void* stream) {
    const std::string fn = "nhans_drift_warp";
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (nclips > 0 && (!eoff || !toff || !a || !b || !ooff || !out))
        return fail(NHANS_EINVAL, fn + ": null offsets, null lines or null output with " + std::to_string(nclips) + " clips to warp");
    int rc = offsets_check(fn, "estimate", eoff, nclips); if (rc) return rc;
    rc = offsets_check(fn, "target", toff, nclips); if (rc) return rc;
    rc = offsets_check(fn, "output", ooff, nclips); if (rc) return rc;
    std::vector<DriftWarp> jobs;
    long long tiles = 0;
    double total = 0.0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t ne = eoff[i + 1] - eoff[i], nt = toff[i + 1] - toff[i];
        if (ne > kMaxResampleClip || nt > kMaxResampleClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(std::max(ne, nt)) + " samples (0 ... 2^31 - 1)");
        rc = line_check(fn, i, a[i], b[i]); if (rc) return rc;
        int64_t lo, hi;
        drift_range(ne, nt, a[i], b[i], &lo, &hi);
        if (ooff[i + 1] - ooff[i] < hi - lo)
            return fail(NHANS_EINVAL, fn + ": output room of clip " + std::to_string(i) + " is " + std::to_string(ooff[i + 1] - ooff[i]) +
                                      " samples, " + std::to_string(hi - lo) + " needed (nhans_drift_range)");
        if (hi == lo) continue;
        if (!est) return null_clip(fn, i, ne);
        jobs.push_back({est + eoff[i], out + ooff[i], (long long)ne, (long long)lo, (long long)(hi - lo), tiles, a[i], b[i]});
        tiles += (hi - lo + kDriftWarpTile - 1) / kDriftWarpTile;
        total += (double)(hi - lo);
    }
    if (tiles > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many samples for one call (split it)");
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (jobs.empty()) return NHANS_OK;
        const double* tab;
        rc = drift_tab_dev(c, &tab); if (rc) return rc;
        DriftWarp* jobs_dev;
        rc = ws_upload(c, jobs, s, &jobs_dev); if (rc) return rc;
        {   // per output 32 taps, two fused multiply-adds each (the coefficient, the sum); it reads about as many samples as it writes
            Prof pr(c, s, "drift_warp");
            launch_drift_warp("drift_warp", jobs_dev, (int)jobs.size(), tiles, tab, s);
            pr.done(8.0 * kDriftT * total, 8.0 * total + 8.0 * (kDriftTableG + kDriftTableD));
        }
        return NHANS_OK;
    });
}

}  // extern "C"
