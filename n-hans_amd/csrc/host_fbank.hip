// ---- filterbank features (include/nhans_hip.h: nhans_fbank_*) ----------------------------------------------------------
// The triangular designer (double, host only), the band table a filterbank becomes -- per band the span between its first
// and last non-zero float32 weight, weights contiguous -- and the one place that turns runs of rows into a launch of
// fbank.hip (fbank_launch): nhans_fbank_rows here and the hook of an online push (host_online.hip) both go through it.
#include "host_internal.h"

namespace {

constexpr double kSlaneyLinHz = 200.0 / 3.0, kSlaneyBreakHz = 1000.0, kSlaneyBreakMel = 15.0;
const double kSlaneyLogStep = std::log(6.4) / 27.0;
constexpr double kF32Max = (double)std::numeric_limits<float>::max();

double hz_to_mel(double f, int scale) {
    if (scale == NHANS_FBANK_HTK) return 2595.0 * std::log10(1.0 + f / 700.0);
    return f < kSlaneyBreakHz ? f / kSlaneyLinHz : kSlaneyBreakMel + std::log(f / kSlaneyBreakHz) / kSlaneyLogStep;
}
double mel_to_hz(double m, int scale) {
    if (scale == NHANS_FBANK_HTK) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    return m < kSlaneyBreakMel ? m * kSlaneyLinHz : kSlaneyBreakHz * std::exp((m - kSlaneyBreakMel) * kSlaneyLogStep);
}

int check_matrix_shape(const char* fn, int n_out) {
    if (n_out < 1 || n_out > kFbankMaxOut)
        return fail(NHANS_EINVAL, std::string(fn) + ": n_out " + std::to_string(n_out) + " outside [1, " + std::to_string(kFbankMaxOut) + "]");
    return NHANS_OK;
}

// w [n_out, 201] (double) -> the table of its float32 rounding.  Refuses what nhans_fbank_open refuses.
int table_build(const char* fn_, const double* w, int n_out, int power, double floor, FbankTable* t) {
    const std::string fn = fn_;
    int rc = check_matrix_shape(fn_, n_out); if (rc) return rc;
    if (!w) return fail(NHANS_EINVAL, fn + ": null argument");
    if (power != 1 && power != 2) return fail(NHANS_EINVAL, fn + ": power must be 1 or 2 (got " + std::to_string(power) + ")");
    if (!(floor > 0.0) || !(floor <= kF32Max) || !((float)floor > 0.f))
        return fail(NHANS_EINVAL, fn + ": floor must be finite and > 0 as a float32");
    std::vector<int32_t> first(n_out, 0), count(n_out, 0), woff(n_out, 0);
    std::vector<float> wt;
    for (int m = 0; m < n_out; ++m) {
        int lo = kBins, hi = -1;
        for (int k = 0; k < kBins; ++k) {
            const double v = w[(size_t)m * kBins + k];
            if (!(v >= 0.0) || !(v <= kF32Max))
                return fail(NHANS_EINVAL, fn + ": weight [" + std::to_string(m) + ", " + std::to_string(k) +
                                          "] is negative or not finite (as a float32)");
            if ((float)v != 0.f) { lo = std::min(lo, k); hi = k; }
        }
        woff[m] = (int32_t)wt.size();
        if (hi < 0) continue;                       // (an empty band: count 0, ln(floor))
        first[m] = lo; count[m] = hi - lo + 1;
        for (int k = lo; k <= hi; ++k) wt.push_back((float)w[(size_t)m * kBins + k]);
    }
    if (wt.size() > (size_t)kFbankMaxSpan)
        return fail(NHANS_EINVAL, fn + ": the bands span " + std::to_string(wt.size()) + " bins together, more than the table's " +
                                  std::to_string(kFbankMaxSpan) + " (NHANS_FBANK_MAX_SPAN)");
    t->n_out = n_out; t->power = power; t->floor = (float)floor; t->nspan = (int)wt.size();
    t->words.clear();
    t->words.insert(t->words.end(), first.begin(), first.end());
    t->words.insert(t->words.end(), count.begin(), count.end());
    t->words.insert(t->words.end(), woff.begin(), woff.end());
    const size_t at = t->words.size();
    t->words.resize(at + wt.size());
    if (!wt.empty()) std::memcpy(t->words.data() + at, wt.data(), wt.size() * sizeof(float));
    t->dev = nullptr;
    return NHANS_OK;
}

}  // namespace

int fbank_table_clone(const FbankTable& from, const char* fn, FbankTable* out) {
    int* dev = nullptr;
    const size_t bytes = from.words.size() * sizeof(int32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), bytes);
    if (e != hipSuccess) return fail(NHANS_ENOMEM, std::string(fn) + ": hipMalloc failed: " + hipGetErrorString(e));
    // (synchronous, from pageable memory: the table is on the device when this returns, whatever stream reads it next)
    e = hipMemcpy(dev, from.words.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dev);
        return fail(NHANS_EHIP, std::string(fn) + ": hipMemcpy: " + hipGetErrorString(e));
    }
    *out = from;
    out->dev = dev;
    return NHANS_OK;
}

void fbank_table_free(FbankTable* t) {
    if (t->dev) (void)hipFree(t->dev);      // (hipFree waits for the device: no launch still reads the table)
    t->dev = nullptr;
}

int fbank_launch(nhans_ctx* c, const FbankTable& t, const char* name, const FbankRows* rows, int nruns, FbankRun* runs_dev,
                 hipStream_t s) {
    std::vector<FbankRun> runs;
    long long tiles = 0, total = 0;
    for (int r = 0; r < nruns; ++r) {
        if (rows[r].nrows <= 0) continue;
        runs.push_back({rows[r].src, rows[r].dst, (long long)rows[r].nrows, tiles});
        tiles += (rows[r].nrows + kFbankTile - 1) / kFbankTile;
        total += rows[r].nrows;
    }
    if (runs.empty()) return NHANS_OK;
    if (tiles > 0x7fffffffLL) return fail(NHANS_EINVAL, std::string(name) + ": too many rows for one launch (split the call)");
    const int rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
    Prof pr(c, s, name);
    launch_fbank(name, runs_dev, (int)runs.size(), tiles, t.dev, t.n_out, t.nspan, t.power, t.floor, s);
    pr.done((double)total * (2.0 * t.nspan + kBins + t.n_out), (double)total * 4.0 * (kBins + t.n_out));
    return NHANS_OK;
}

// ================================================================================================
extern "C" {

int nhans_fbank_design(int n_out, double f_min, double f_max, int scale, int norm, double* w_out) {
    const std::string fn = "nhans_fbank_design";
    const int rc = check_matrix_shape("nhans_fbank_design", n_out); if (rc) return rc;
    if (!(f_min >= 0.0) || !(f_max <= 8000.0) || !(f_min < f_max))
        return fail(NHANS_EINVAL, fn + ": needs 0 <= f_min < f_max <= 8000 Hz");
    if (scale != NHANS_FBANK_HTK && scale != NHANS_FBANK_SLANEY)
        return fail(NHANS_EINVAL, fn + ": scale must be NHANS_FBANK_HTK or NHANS_FBANK_SLANEY");
    if (norm != NHANS_FBANK_NORM_NONE && norm != NHANS_FBANK_NORM_SLANEY)
        return fail(NHANS_EINVAL, fn + ": norm must be NHANS_FBANK_NORM_NONE or NHANS_FBANK_NORM_SLANEY");
    const double m0 = hz_to_mel(f_min, scale), m1 = hz_to_mel(f_max, scale);
    std::vector<double> p(n_out + 2);
    for (int i = 0; i < n_out + 2; ++i) p[i] = mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(n_out + 1), scale);
    int empty = 0;
    for (int m = 0; m < n_out; ++m) {
        const double up = p[m + 1] - p[m], down = p[m + 2] - p[m + 1];
        const double gain = norm == NHANS_FBANK_NORM_SLANEY ? 2.0 / (p[m + 2] - p[m]) : 1.0;
        bool any = false;
        for (int k = 0; k < kBins; ++k) {
            const double f = 40.0 * k;
            const double v = std::max(0.0, std::min((f - p[m]) / up, (p[m + 2] - f) / down)) * gain;
            if ((float)v != 0.f) any = true;
            if (w_out) w_out[(size_t)m * kBins + k] = v;
        }
        empty += any ? 0 : 1;
    }
    return empty;
}

int nhans_fbank_open(nhans_ctx* c, const double* w, int n_out, int power, double floor, void* stream, nhans_fbank** out) {
    if (!out) return fail(NHANS_EINVAL, "nhans_fbank_open: null argument");
    *out = nullptr;
    // (the matrix first: what it refuses needs no device)
    FbankTable host;
    int rc = table_build("nhans_fbank_open", w, n_out, power, floor, &host); if (rc) return rc;
    return ctx_call(c, stream, [&](hipStream_t) -> int {
        nhans_fbank* fb = new nhans_fbank();
        fb->c = c; fb->device = c->device;
        rc = fbank_table_clone(host, "nhans_fbank_open", &fb->t);
        if (rc) { delete fb; return rc; }
        *out = fb;
        return NHANS_OK;
    });
}

void nhans_fbank_close(nhans_fbank* fb) {
    if (!fb) return;
    (void)hipSetDevice(fb->device);
    fbank_table_free(&fb->t);
    delete fb;
}

int nhans_fbank_rows(nhans_fbank* fb, const float* logmag, int64_t nrows, float* out, void* stream) {
    return object_call(fb, "nhans_fbank_rows: null object", stream, [&](hipStream_t s) {
        if (nrows < 0) return fail(NHANS_EINVAL, "nhans_fbank_rows: negative row count");
        if (nrows == 0) return (int)NHANS_OK;
        if (!logmag || !out) return fail(NHANS_EINVAL, "nhans_fbank_rows: null buffer");
        WsPlan p;
        FbankRun* runs_dev;     // (fbank_launch fills and copies the one run)
        p.add(&runs_dev, 1);
        const int rc = ws_commit(fb->c, p); if (rc) return rc;
        const FbankRows rows{logmag, out, nrows};
        return fbank_launch(fb->c, fb->t, "fbank_rows", &rows, 1, runs_dev, s);
    });
}

}  // extern "C"
