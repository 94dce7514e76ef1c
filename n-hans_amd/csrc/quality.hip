// LLR, cepstral distance and frequency-weighted segmental SNR of an estimate y against a clean target x on the device
// (include/nhans_hip.h: nhans_quality, where the definition is stated operation by operation).
// Both signals are float32 at 16 kHz, n common samples, frames of 480 at hop 120; every operation is in double.
//
//   1. quality_lpc     a workgroup takes kQualityLpcTile consecutive frames of one clip.  The tile's span of both signals
//                      (480 + 6 * 120 samples) is staged in LDS once, as doubles, with the window beside it.  Thread c <
//                      frames * 34 owns one autocorrelation chain (frame, signal, lag k): one __fma_rn chain over i
//                      ascending of the two windowed samples, each windowed by one __dmul_rn as it is read.  Then one lane
//                      per (frame, signal) runs the Levinson-Durbin recursion and the cepstrum recursion, one lane per
//                      (frame, den | num) a quadratic form, one lane per frame the distance and the two clamped values.
//   2. quality_bands   a wavefront per (frame, signal): the 512-point transform (fft512.h) of the windowed frame, |X_k| for
//                      k <= 256, then one lane per band the band sum over k ascending, one lane per band s_j and g_j,
//                      lane 0 the weighted mean over j ascending.  Two transforms a frame, not one of x_w + i y_w
//                      separated by symmetry: the separated spectrum of an all-zero target is zero only up to the
//                      transform's rounding of the estimate, and the rule that skips a frame (G == 0) is exact.
//   3. quality_finish  one workgroup per clip: the three means (one lane each, a __dadd_rn chain over the kept frames,
//                      f ascending), then per figure of LLR and CD the q-th smallest kept value by a radix select on the
//                      bit patterns (eight passes of eight bits, most significant first, a 256-bin histogram of integer
//                      atomics in LDS), the chain over the frames below it, f ascending, and the record.
//
// LDS layout of quality_lpc: the target's span at doubles [0, 1200), the estimate's at [1201, 2401).  The lanes of a frame's
// 34 chains read x[i + k] at consecutive doubles (lags 0 ... 16 of the target, then of the estimate) and x[i] as a
// broadcast.  A bank is 4 bytes and 32 lanes of an 8-byte access take the 64 banks once when their doubles differ mod 32:
// with the estimate 1201 = 17 (mod 32) doubles after the target, the first 32 lanes of a frame -- 17 lags of the target,
// 15 of the estimate -- fall on 32 different doubles mod 32 (an offset of 1200 = 16 (mod 32) would put 15 of them on the
// banks of the target's).  A frame's remaining two lanes share a pass with the next frame's (120 = 24 mod 32 doubles on):
// at most two of them meet.
//
// No floating-point atomics and no reduction whose shape depends on the batch: a record and every per-frame value have the
// same bits alone or in any batch, at any offset, on every run.  Samples are fetched with single 4-byte loads and only
// inside [0, n) of a clip.
#include "score_common.h"
#include "fft512.h"

#include <algorithm>
#include <cmath>

namespace nhans {

namespace {

constexpr int QP = kQualityOrder, QP1 = kQualityOrder + 1, QN = kQualityFrame, QH = kQualityHop;
constexpr int kSpan = QN + (kQualityLpcTile - 1) * QH;      // 1200
constexpr int kEstAt = kSpan + 1;                           // 17 (mod 32): see above
static_assert(kEstAt % 32 == 17, "the estimate's span sits 17 (mod 32) doubles after the target's");
static_assert(kQualityLpcTile * 2 * QP1 <= 256, "one thread per autocorrelation chain");
static_assert(kQualityFft == 512 && kQualityBandTile == 2 && kQualityMaxBands <= 64, "the band launch's shape");

__device__ __forceinline__ bool q_pos_finite(double v) { return v > 0.0 && v < __longlong_as_double(0x7ff0000000000000LL); }

__global__ void __launch_bounds__(256) quality_lpc_kernel(const QualityRun* __restrict__ runs, int nruns, const double* __restrict__ tab,
                                                          double* __restrict__ vals, double* __restrict__ lpc_out) {
    __shared__ double sig[kEstAt + kSpan];
    __shared__ double win[QN];
    __shared__ double r[kQualityLpcTile][2][QP1];
    __shared__ double a[kQualityLpcTile][2][QP1];
    __shared__ double cep[kQualityLpcTile][2][QP1];
    __shared__ double nw[kQualityLpcTile][2][QP1];
    __shared__ double quad[kQualityLpcTile][2];
    __shared__ int ok[kQualityLpcTile][2];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const QualityRun run = runs[find_run<QualityRun, &QualityRun::ltile0>(runs, nruns, b)];
    const long long f0 = (b - run.ltile0) * kQualityLpcTile;
    const int nf = (int)(run.frames - f0 < kQualityLpcTile ? run.frames - f0 : kQualityLpcTile);     // >= 1
    const int span = QN + (nf - 1) * QH;                    // f0 * 120 + span <= n
    const float* __restrict__ xt = run.tgt + f0 * QH;
    const float* __restrict__ xe = run.est + f0 * QH;
    for (int i = tid; i < span; i += 256) {
        sig[i] = (double)xt[i];
        sig[kEstAt + i] = (double)xe[i];
    }
    for (int i = tid; i < QN; i += 256) win[i] = tab[i];
    __syncthreads();
    // ---- r[k] = sum_i xw[i] xw[i + k]: thread -> (frame, signal, lag)
    const int cf = tid / (2 * QP1), crem = tid - cf * 2 * QP1, csg = crem / QP1, ck = crem - csg * QP1;
    const bool chain = tid < nf * 2 * QP1;
    if (chain) {
        const double* x = sig + csg * kEstAt + cf * QH;
        double acc = 0.0;
        for (int i = 0; i < QN - ck; ++i) acc = __fma_rn(__dmul_rn(x[i], win[i]), __dmul_rn(x[i + ck], win[i + ck]), acc);
        r[cf][csg][ck] = acc;
    }
    __syncthreads();
    // ---- Levinson-Durbin and the cepstrum: lane -> (frame, signal)
    if (tid < nf * 2) {
        const int f = tid >> 1, sg = tid & 1;
        const double* rr = r[f][sg];
        double* aa = a[f][sg];
        double* nn = nw[f][sg];
        double* cc = cep[f][sg];
        bool good = rr[0] != 0.0;
        double E = rr[0];
        aa[0] = 1.0;
        for (int m = 1; m <= QP && good; ++m) {
            double acc = rr[m];
            for (int j = 1; j < m; ++j) acc = __fma_rn(aa[j], rr[m - j], acc);
            const double k = -__ddiv_rn(acc, E);
            for (int j = 1; j < m; ++j) nn[j] = __fma_rn(k, aa[m - j], aa[j]);
            for (int j = 1; j < m; ++j) aa[j] = nn[j];
            aa[m] = k;
            E = __dmul_rn(E, __fma_rn(-k, k, 1.0));
            good = q_pos_finite(E);
        }
        cc[0] = 0.0;
        if (good) {
            for (int m = 1; m <= QP; ++m) {
                double s = 0.0;
                for (int k = 1; k < m; ++k) s = __fma_rn(__dmul_rn(__ddiv_rn((double)k, (double)m), cc[k]), aa[m - k], s);
                cc[m] = __dsub_rn(-aa[m], s);
            }
        } else {
            for (int m = 1; m <= QP; ++m) { aa[m] = quiet_nan(); cc[m] = quiet_nan(); }
        }
        ok[f][sg] = good ? 1 : 0;
    }
    __syncthreads();
    // ---- the quadratic forms on the TARGET's matrix: lane -> (frame, 0: den = a_t' R_t a_t | 1: num = a_e' R_t a_e)
    if (tid < nf * 2) {
        const int f = tid >> 1, wh = tid & 1;
        const double* rt = r[f][0];
        const double* av = a[f][wh];
        double q = 0.0;
        for (int i = 0; i <= QP; ++i) {
            double row = 0.0;
            for (int j = 0; j <= QP; ++j) row = __fma_rn(rt[i > j ? i - j : j - i], av[j], row);
            q = __fma_rn(av[i], row, q);
        }
        quad[f][wh] = q;
    }
    __syncthreads();
    if (tid < nf) {
        const int f = tid;
        const double den = quad[f][0], num = quad[f][1];
        const bool good = ok[f][0] && ok[f][1] && q_pos_finite(den) && q_pos_finite(num);
        double dc2 = 0.0;
        for (int m = 1; m <= QP; ++m) {
            const double t = __dsub_rn(cep[f][0][m], cep[f][1][m]);
            dc2 = __fma_rn(t, t, dc2);
        }
        double llr = quiet_nan(), cd = quiet_nan();
        if (good) {
            llr = __dadd_rn(fmin(fmax(log(__ddiv_rn(num, den)), 0.0), kQualityLlrMax), 0.0);
            cd = __dadd_rn(fmin(fmax(__dmul_rn(kQualityCdScale, __dsqrt_rn(__dmul_rn(2.0, dc2))), 0.0), kQualityCdMax), 0.0);
        }
        double* o = vals + (size_t)(run.frame0 + f0 + f) * 3;
        o[0] = llr; o[1] = cd;
        if (lpc_out) {
            double* row = lpc_out + (size_t)(run.frame0 + f0 + f) * kQualityLpcFields;
            row[4 * QP1] = num; row[4 * QP1 + 1] = den; row[4 * QP1 + 2] = dc2; row[4 * QP1 + 3] = 0.0;
        }
    }
    if (lpc_out && chain) {
        double* row = lpc_out + (size_t)(run.frame0 + f0 + cf) * kQualityLpcFields;
        row[csg * QP1 + ck] = r[cf][csg][ck];
        row[2 * QP1 + csg * QP1 + ck] = a[cf][csg][ck];
    }
}

// One workgroup: kQualityBandTile frames of one clip, a wavefront per (frame, signal): waves 0 and 1 the target and the
// estimate of the first, waves 2 and 3 of the second.  A wavefront without a frame runs the transform on zeros: its
// barriers are the workgroup's.
__global__ void __launch_bounds__(256) quality_bands_kernel(const QualityRun* __restrict__ runs, int nruns, const double* __restrict__ tab,
                                                            const double* __restrict__ W, const int* __restrict__ span, int K,
                                                            double* __restrict__ vals) {
    __shared__ double tw[2 * kQualityFft];                  // cos, then -sin
    __shared__ double buf[2 * kQualityBandTile][2][kFft512Buf];
    __shared__ double mag[2 * kQualityBandTile][kQualityBins + 1];
    __shared__ double bs[kQualityBandTile][2][kQualityMaxBands];     // X_j and Y_j, then (the same lane, in place) g_j and 35 - s_j
    const int tid = threadIdx.x, j = tid & 63, wave = tid >> 6, fr = wave >> 1, sg = wave & 1;
    const long long b = blockIdx.x;
    const QualityRun run = runs[find_run<QualityRun, &QualityRun::btile0>(runs, nruns, b)];
    const long long f = (b - run.btile0) * kQualityBandTile + fr;
    const bool active = f < run.frames;
    for (int t = tid; t < 2 * kQualityFft; t += 256) tw[t] = tab[QN + t];
    Fft512C v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = {0.0, 0.0};
    if (active) {
        const float* __restrict__ x = (sg ? run.est : run.tgt) + f * QH;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = j + 64 * q;
            if (i < QN) v[q].r = __dmul_rn((double)x[i], tab[i]);
        }
    }
    fft512_wave(j, tw, tw + kQualityFft, v, buf[wave][0], buf[wave][1]);
    // thread j holds bins j + 64 q; the bands read bins 0 ... 256
#pragma unroll
    for (int q = 0; q < 4; ++q) mag[wave][j + 64 * q] = __dsqrt_rn(__fma_rn(v[q].i, v[q].i, __dmul_rn(v[q].r, v[q].r)));
    if (j == 0) mag[wave][256] = __dsqrt_rn(__fma_rn(v[4].i, v[4].i, __dmul_rn(v[4].r, v[4].r)));
    __syncthreads();
    if (j < K) {                                            // band sums: lane j of the signal's wavefront owns band j
        const double* __restrict__ w = W + (size_t)j * kQualityBins;
        const double* m = mag[wave];
        double acc = 0.0;
        // [span[2 j], span[2 j + 1]): the bins from the row's first non-zero weight to its last.  The chain over all 257 bins
        // has the same bits: a zero weight adds fma(0, |X_k|, acc) = acc, and acc is never -0
        for (int k = span[2 * j]; k < span[2 * j + 1]; ++k) acc = __fma_rn(w[k], m[k], acc);
        bs[fr][sg][j] = acc;
    }
    __syncthreads();
    if (sg == 0 && j < K) {
        const double X = bs[fr][0][j], Y = bs[fr][1][j];
        double s = kQualitySnrMax;
        if (X != Y) {
            const double d = __dsub_rn(X, Y);
            s = __dmul_rn(10.0, log10(__ddiv_rn(__dmul_rn(X, X), __dmul_rn(d, d))));
            s = fmin(fmax(s, kQualitySnrMin), kQualitySnrMax);
        }
        bs[fr][0][j] = pow(X, kQualityGamma);
        bs[fr][1][j] = __dsub_rn(kQualitySnrMax, s);           // the band's deficit: 0 where it is clamped at the top
    }
    __syncthreads();
    if (active && sg == 0 && j == 0) {
        double G = 0.0, S = 0.0;
        for (int q = 0; q < K; ++q) {
            G = __dadd_rn(G, bs[fr][0][q]);
            S = __fma_rn(bs[fr][0][q], bs[fr][1][q], S);
        }
        // 35 less the weighted mean of the deficits: equal signals give 35 exactly
        vals[(size_t)(run.frame0 + f) * 3 + 2] = G == 0.0 ? quiet_nan() : __dsub_rn(kQualitySnrMax, __ddiv_rn(S, G));
    }
}

// One workgroup per clip.
__global__ void __launch_bounds__(256) quality_finish_kernel(const QualityRun* __restrict__ runs, const double* __restrict__ vals,
                                                             double* __restrict__ rec) {
    __shared__ unsigned hist[256];
    __shared__ double sum[3], thr[2];
    __shared__ long long kept[3], below[2];
    __shared__ unsigned long long s_prefix;
    __shared__ long long s_want, s_below;
    const int tid = threadIdx.x;
    const QualityRun run = runs[blockIdx.x];
    const long long M = run.frames;
    const double* __restrict__ v = vals + (size_t)run.frame0 * 3;
    if (tid < 3) {
        double a = 0.0;
        long long n = 0;
        for (long long f = 0; f < M; ++f) {
            const double x = v[3 * f + tid];
            if (x == x) { a = __dadd_rn(a, x); ++n; }
        }
        sum[tid] = a; kept[tid] = n;
    }
    __syncthreads();
    const long long Mk = kept[0], q = (19 * Mk + 10) / 20;
    if (Mk > 0) {
        for (int fig = 0; fig < 2; ++fig) {
            if (tid == 0) { s_prefix = 0ULL; s_want = q; s_below = 0; }
            for (int pass = 7; pass >= 0; --pass) {
                const int shift = 8 * pass;
                hist[tid] = 0u;
                __syncthreads();
                const unsigned long long prefix = s_prefix, mask = pass == 7 ? 0ULL : ~0ULL << (shift + 8);
                for (long long f = tid; f < M; f += 256) {
                    const double x = v[3 * f + fig];
                    if (x == x) {
                        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
                        if ((bits & mask) == prefix) atomicAdd(&hist[(unsigned)(bits >> shift) & 255u], 1u);
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    long long cum = 0, want = s_want;
                    for (int d = 0; d < 256; ++d) {
                        const long long h = hist[d];
                        if (cum + h >= want) {
                            s_prefix = prefix | ((unsigned long long)d << shift);
                            s_want = want - cum;
                            s_below += cum;
                            break;
                        }
                        cum += h;
                    }
                }
                __syncthreads();
            }
            if (tid == 0) { thr[fig] = __longlong_as_double((long long)s_prefix); below[fig] = s_below; }
            __syncthreads();
        }
    }
    double* o = rec + (size_t)blockIdx.x * kQualityFields;
    if (tid < 2) {
        double m = quiet_nan(), m95 = quiet_nan();
        if (Mk > 0) {
            const double t = thr[tid];
            double a = 0.0;
            for (long long f = 0; f < M; ++f) {
                const double x = v[3 * f + tid];
                if (x < t) a = __dadd_rn(a, x);
            }
            m95 = __ddiv_rn(__dadd_rn(a, __dmul_rn((double)(q - below[tid]), t)), (double)q);
            m = __ddiv_rn(sum[tid], (double)Mk);
        }
        o[4 + 2 * tid] = m; o[5 + 2 * tid] = m95;
    }
    if (tid == 2) {
        o[0] = (double)run.n; o[1] = (double)M; o[2] = (double)Mk; o[3] = (double)kept[2];
        o[8] = kept[2] > 0 ? __ddiv_rn(sum[2], (double)kept[2]) : quiet_nan();
        for (int i = 9; i < kQualityFields; ++i) o[i] = 0.0;
    }
}

double q_hz_to_mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
double q_mel_to_hz(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

}  // namespace

void quality_table(double* tab) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < kQualityFrame; ++i) tab[i] = 0.5 - 0.5 * std::cos(2.0 * pi * (double)(i + 1) / (double)(kQualityFrame + 1));
    fft512_twiddles(tab + kQualityFrame);
}

// kQualityBands triangles on the HTK mel scale between 0 and 8000 Hz over the bins 31.25 k: the construction of
// nhans_fbank_design (HTK, no normalisation) on 257 bins
void quality_default_bands(double* w) {
    const double m0 = q_hz_to_mel(0.0), m1 = q_hz_to_mel(8000.0);
    double p[kQualityBands + 2];
    for (int i = 0; i < kQualityBands + 2; ++i) p[i] = q_mel_to_hz(m0 + (m1 - m0) * (double)i / (double)(kQualityBands + 1));
    for (int m = 0; m < kQualityBands; ++m) {
        const double up = p[m + 1] - p[m], down = p[m + 2] - p[m + 1];
        for (int k = 0; k < kQualityBins; ++k) {
            const double f = 31.25 * k;
            w[(size_t)m * kQualityBins + k] = std::max(0.0, std::min((f - p[m]) / up, (p[m + 2] - f) / down));
        }
    }
}

void launch_quality_lpc(const char* kernel, const QualityRun* runs_dev, int nruns, long long ntiles, const double* tab, double* vals,
                        double* lpc_out, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    NHANS_LAUNCH(kernel, quality_lpc_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, tab, vals, lpc_out);
}

void launch_quality_bands(const char* kernel, const QualityRun* runs_dev, int nruns, long long ntiles, const double* tab,
                          const double* bands, const int* span, int nbands, double* vals, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    if (nbands < 1 || nbands > kQualityMaxBands) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, quality_bands_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, tab, bands, span, nbands, vals);
}

void launch_quality_finish(const char* kernel, const QualityRun* runs_dev, int nruns, const double* vals, double* rec, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, quality_finish_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, vals, rec);
}

}  // namespace nhans
