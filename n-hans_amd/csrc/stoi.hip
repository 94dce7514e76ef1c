// STOI and extended STOI of an estimate y against a clean target x on the device (include/nhans_hip.h: nhans_stoi, where
// the definition is stated in full).  Both signals are float32 at 10 kHz, n common samples; every
// operation is in double.
//
//   1. stoi_power     P_m = sum (w x_m)^2 of every frame m < M0 of the TARGET (256 samples at hop 128, w = hanning(256)).
//   2. stoi_keep      per clip: P_max, the keep mask P_m > P_max * 1e-4 and its exclusive scan -> the list of kept frames
//                     and their count Mk.  A maximum and integers: exact.
//   3. stoi_bands     per analysis frame q < Mk - 1 and signal: the 256 samples [128 q, 128 q + 256) of the kept windowed
//                     frames overlap-added at hop 128 -- kept frame q plus kept frame q - 1 (first half) or q + 1 (second
//                     half); the joined signal is never stored --, windowed again, zero-padded to 512 and transformed
//                     (fft512.h), then B[j][q] = sqrt(sum_{k in band j} |X_q(k)|^2) for the 15 third-octave bands.
//   4. stoi_segments  per segment s < Mk - 30 (columns s ... s + 29 of both band tensors): d_s and e_s.
//   5. stoi_finish    per clip: stoi = (sum_s d_s) / S, estoi likewise; NaN where S == 0.
//
// The order of every sum is fixed relative to the clip's first sample, so a record's bits are a property of the clip pair
// -- not of its place in the batch, its neighbours, the alignment of its first sample or the run:
//   * a frame's power: lane l of one wavefront adds its terms of samples l, l + 64, l + 128, l + 192 in that order (one
//     __fma_rn from +0.0 each), then the __shfl_down tree 32, ..., 1 in __dadd_rn;
//   * a sample of the joined signal is a sum of two terms (one for the first half of analysis frame 0); the transform is
//     one fixed sequence of operations per frame; a band's sum adds its bins |X(k)|^2 one after the other, k ascending;
//   * a segment is worked by 16 lanes, lane j < 15 owning band j: every sum over the 30 columns is one chain in column
//     order, every sum over the 15 bands the __shfl_xor tree 8, 4, 2, 1 (both partners of a step add the same two values,
//     so all lanes hold the same bits), the column terms of e_s are added one after the other in column order;
//   * a clip's two means add its segments' figures one after the other, s ascending (through LDS in rounds of 256), and
//     divide once.
// No floating-point atomics, and no reduction whose shape depends on the batch.  Samples are fetched with single 4-byte
// loads, so an odd offset changes nothing.
#include "score_common.h"
#include "fft512.h"

#include <cmath>

namespace nhans {

namespace {

constexpr double kStoiEps = 2.220446049250313e-16;          // 2^-52
constexpr double kStoiClip = 6.623413251903491;             // 1 + 10^(15/20)
constexpr double kStoiRange = 1e-4;                         // 40 dB

// third-octave bands from 150 Hz as bins [lo, hi) of the 512-point transform at 10 kHz: band j is [kBandEdge[j], kBandEdge[j + 1])
__constant__ int kBandEdge[kStoiBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// the sum over the 16 lanes of a segment's group, in every one of them
__device__ __forceinline__ double group_all(double v) {
    for (int off = 8; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off, 16));
    return v;
}

// One wavefront per frame of the target.
__global__ void __launch_bounds__(256) stoi_power_kernel(const StoiRun* __restrict__ runs, int nruns, const double* __restrict__ tab,
                                                         double* __restrict__ power) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.x;
    const StoiRun run = runs[find_run<StoiRun, &StoiRun::ptile0>(runs, nruns, b)];
    const long long m = (b - run.ptile0) * kStoiPowerTile + wave;
    if (m >= run.frames) return;
    const float* __restrict__ x = run.tgt + m * kStoiHop;
    double a = 0.0;
    for (int j = 0; j < kStoiFrame / 64; ++j) {
        const int i = lane + 64 * j;
        const double v = __dmul_rn(tab[i], (double)x[i]);
        a = __fma_rn(v, v, a);
    }
    a = wave_sum(a);
    if (lane == 0) power[run.frame0 + m] = a;
}

// One workgroup per clip: the maximum, the mask, its scan.
__global__ void __launch_bounds__(256) stoi_keep_kernel(const StoiRun* __restrict__ runs, const double* __restrict__ power,
                                                        int* __restrict__ kept, long long* __restrict__ nkept) {
    __shared__ double red[256];
    __shared__ int scan[2][256];
    const int tid = threadIdx.x;
    const StoiRun run = runs[blockIdx.x];
    const double* __restrict__ p = power + run.frame0;
    double mx = 0.0;
    for (long long m = tid; m < run.frames; m += 256) mx = fmax(mx, p[m]);
    red[tid] = mx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] = fmax(red[tid], red[tid + off]);
        __syncthreads();
    }
    const double thr = __dmul_rn(red[0], kStoiRange);
    long long base = 0;
    for (long long m0 = 0; m0 < run.frames; m0 += 256) {
        const long long m = m0 + tid;
        const int keep = m < run.frames && p[m] > thr ? 1 : 0;
        int cur = 0;
        scan[0][tid] = keep;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {           // inclusive scan, two buffers in turn
            const int v = scan[cur][tid] + (tid >= off ? scan[cur][tid - off] : 0);
            scan[1 - cur][tid] = v;
            cur = 1 - cur;
            __syncthreads();
        }
        if (keep) kept[run.frame0 + base + scan[cur][tid] - 1] = (int)m;
        base += scan[cur][255];
        __syncthreads();
    }
    if (tid == 0) nkept[blockIdx.x] = base;
}

// sample i of analysis frame q of one signal: w[i] (w[i] x_q[i] + w[i'] x_q'[i']), (q', i') = (q - 1, i + 128) in the first
// half and (q + 1, i - 128) in the second, x_q the q-th KEPT frame
__device__ __forceinline__ double analysis_sample(const float* __restrict__ x, const int* __restrict__ kept, long long q, int i,
                                                  const double* __restrict__ w) {
    const double own = __dmul_rn(w[i], (double)x[(long long)kept[q] * kStoiHop + i]);
    double other = 0.0;
    if (i >= kStoiHop) other = __dmul_rn(w[i - kStoiHop], (double)x[(long long)kept[q + 1] * kStoiHop + i - kStoiHop]);
    else if (q > 0) other = __dmul_rn(w[i + kStoiHop], (double)x[(long long)kept[q - 1] * kStoiHop + i + kStoiHop]);
    return __dmul_rn(w[i], __dadd_rn(own, other));
}

// One workgroup: kStoiBandTile analysis frames of one clip, a wavefront per (frame, signal): waves 0 and 1 the target and
// the estimate of the first, waves 2 and 3 of the second.  A wavefront without a frame runs the transform on zeros: its
// barriers are the workgroup's.
__global__ void __launch_bounds__(256) stoi_bands_kernel(const StoiRun* __restrict__ runs, int nruns, const double* __restrict__ tab,
                                                         const int* __restrict__ kept, const long long* __restrict__ nkept,
                                                         double* __restrict__ bands, long long rows) {
    __shared__ double tw[2 * kStoiFft];                     // cos, then -sin
    __shared__ double buf[4][2][kFft512Buf];
    const int tid = threadIdx.x, j = tid & 63, wave = tid >> 6, sig = wave & 1;
    const long long b = blockIdx.x;
    const int ri = find_run<StoiRun, &StoiRun::btile0>(runs, nruns, b);
    const StoiRun run = runs[ri];
    const long long q = (b - run.btile0) * kStoiBandTile + (wave >> 1);
    const bool active = q < nkept[ri] - 1;
    for (int t = tid; t < 2 * kStoiFft; t += 256) tw[t] = tab[kStoiFrame + t];
    double* re = buf[wave][0];
    Fft512C v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = {0.0, 0.0};
    if (active) {
        const float* __restrict__ x = sig ? run.est : run.tgt;
        const int* __restrict__ kp = kept + run.frame0;
#pragma unroll
        for (int r = 0; r < kStoiFrame / 64; ++r) v[r].r = analysis_sample(x, kp, q, j + 64 * r, tab);
    }
    fft512_wave(j, tw, tw + kStoiFft, v, re, buf[wave][1]);
    // thread j holds bins j + 64 r; the bands end at bin 218
#pragma unroll
    for (int r = 0; r < 4; ++r) re[j + 64 * r] = __fma_rn(v[r].i, v[r].i, __dmul_rn(v[r].r, v[r].r));
    __syncthreads();
    if (active && j < kStoiBands) {
        double a = 0.0;
        for (int k = kBandEdge[j]; k < kBandEdge[j + 1]; ++k) a = __dadd_rn(a, re[k]);
        bands[((size_t)sig * rows + run.band0 + q) * kStoiBands + j] = sqrt(a);
    }
}

// One workgroup: kStoiSegTile segments of one clip, 16 lanes each, lane j < 15 owning band j (lane 15 works on zeros).
__global__ void __launch_bounds__(256) stoi_segments_kernel(const StoiRun* __restrict__ runs, int nruns, const long long* __restrict__ nkept,
                                                            const double* __restrict__ bands, long long rows, double* __restrict__ segs,
                                                            double* __restrict__ segs_out) {
    constexpr int N = kStoiSegment;
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    const long long b = blockIdx.x;
    const int ri = find_run<StoiRun, &StoiRun::stile0>(runs, nruns, b);
    const StoiRun run = runs[ri];
    const long long s = (b - run.stile0) * kStoiSegTile + g;
    if (s >= nkept[ri] - N) return;             // (the whole group: no barrier in this kernel)
    const bool band = l < kStoiBands;
    const double* __restrict__ px = bands + (size_t)(run.band0 + s) * kStoiBands + (band ? l : 0);
    const double* __restrict__ py = px + (size_t)rows * kStoiBands;
    double x[N], y[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        x[q] = band ? px[q * kStoiBands] : 0.0;
        y[q] = band ? py[q * kStoiBands] : 0.0;
    }
    // ---- the band's rows: norms, means
    double sxx = 0.0, syy = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        sxx = __fma_rn(x[q], x[q], sxx); syy = __fma_rn(y[q], y[q], syy);
        sx = __dadd_rn(sx, x[q]); sy = __dadd_rn(sy, y[q]);
    }
    const double alpha = sqrt(sxx) / __dadd_rn(sqrt(syy), kStoiEps);
    const double mx = sx / (double)N, my = sy / (double)N;
    double sc = 0.0;
#pragma unroll
    for (int q = 0; q < N; ++q) sc = __dadd_rn(sc, fmin(__dmul_rn(alpha, y[q]), __dmul_rn(kStoiClip, x[q])));
    const double mc = sc / (double)N;
    double cxx = 0.0, cyy = 0.0, ccc = 0.0, cxc = 0.0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double dx = __dsub_rn(x[q], mx), dy = __dsub_rn(y[q], my);
        const double dc = __dsub_rn(fmin(__dmul_rn(alpha, y[q]), __dmul_rn(kStoiClip, x[q])), mc);
        cxx = __fma_rn(dx, dx, cxx); cyy = __fma_rn(dy, dy, cyy);
        ccc = __fma_rn(dc, dc, ccc); cxc = __fma_rn(dx, dc, cxc);
    }
    const double nx = __dadd_rn(sqrt(cxx), kStoiEps), ny = __dadd_rn(sqrt(cyy), kStoiEps), nc = __dadd_rn(sqrt(ccc), kStoiEps);
    // ---- STOI: the correlation of the centred row of x with that of the clipped y, over the bands
    const double d = group_all(cxc / __dmul_rn(nx, nc)) / (double)kStoiBands;
    // ---- extended STOI: rows normalised, then columns
    double e = 0.0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double xr = __dsub_rn(x[q], mx) / nx, yr = __dsub_rn(y[q], my) / ny;
        const double cx = group_all(xr) / (double)kStoiBands, cy = group_all(yr) / (double)kStoiBands;
        const double ux = band ? __dsub_rn(xr, cx) : 0.0, uy = band ? __dsub_rn(yr, cy) : 0.0;
        const double pxx = group_all(__dmul_rn(ux, ux)), pyy = group_all(__dmul_rn(uy, uy)), pxy = group_all(__dmul_rn(ux, uy));
        e = __dadd_rn(e, pxy / __dmul_rn(__dadd_rn(sqrt(pxx), kStoiEps), __dadd_rn(sqrt(pyy), kStoiEps)));
    }
    e = e / (double)N;
    if (l == 0) {
        const size_t o = 2 * (size_t)(run.seg0 + s);
        segs[o] = d; segs[o + 1] = e;
        if (segs_out) { segs_out[o] = d; segs_out[o + 1] = e; }
    }
}

// One workgroup per clip: the means of its segments' figures, ascending, and the record.
__global__ void __launch_bounds__(256) stoi_finish_kernel(const StoiRun* __restrict__ runs, const long long* __restrict__ nkept,
                                                          const double* __restrict__ segs, double* __restrict__ rec) {
    __shared__ double buf[2][256];
    const int tid = threadIdx.x;
    const StoiRun run = runs[blockIdx.x];
    const long long mk = nkept[blockIdx.x];
    const long long S = mk >= kStoiSegment + 1 ? mk - kStoiSegment : 0;
    double a = 0.0;
    for (long long sb = 0; sb < S; sb += 256) {
        const int nb = (int)(S - sb < 256 ? S - sb : 256);
        if (tid < nb) {
            const size_t o = 2 * (size_t)(run.seg0 + sb + tid);
            buf[0][tid] = segs[o]; buf[1][tid] = segs[o + 1];
        }
        __syncthreads();
        if (tid < 2) {
#pragma unroll 8
            for (int k = 0; k < nb; ++k) a = __dadd_rn(a, buf[tid][k]);
        }
        __syncthreads();
    }
    double* o = rec + (size_t)blockIdx.x * kStoiFields;
    const double nan = quiet_nan();
    if (tid < 2) o[4 + tid] = S > 0 ? a / (double)S : nan;
    if (tid == 2) { o[0] = (double)run.n; o[1] = (double)run.frames; o[2] = (double)mk; o[3] = (double)S; o[6] = 0.0; o[7] = 0.0; }
}

}  // namespace

void stoi_table(double* tab) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < kStoiFrame; ++i) tab[i] = 0.5 * (1.0 - std::cos(2.0 * pi * (double)(i + 1) / (double)(kStoiFrame + 1)));
    fft512_twiddles(tab + kStoiFrame);
}

void launch_stoi_power(const char* kernel, const StoiRun* runs_dev, int nruns, long long ntiles, const double* tab, double* power,
                       hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    NHANS_LAUNCH(kernel, stoi_power_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, tab, power);
}

void launch_stoi_keep(const char* kernel, const StoiRun* runs_dev, int nruns, const double* power, int* kept, long long* nkept,
                      hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, stoi_keep_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, power, kept, nkept);
}

void launch_stoi_bands(const char* kernel, const StoiRun* runs_dev, int nruns, long long ntiles, const double* tab, const int* kept,
                       const long long* nkept, double* bands, long long rows, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    NHANS_LAUNCH(kernel, stoi_bands_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, tab, kept, nkept, bands, rows);
}

void launch_stoi_segments(const char* kernel, const StoiRun* runs_dev, int nruns, long long ntiles, const long long* nkept,
                          const double* bands, long long rows, double* segs, double* segs_out, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    NHANS_LAUNCH(kernel, stoi_segments_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, nkept, bands, rows, segs,
                 segs_out);
}

void launch_stoi_finish(const char* kernel, const StoiRun* runs_dev, int nruns, const long long* nkept, const double* segs, double* rec,
                        hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, stoi_finish_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, nkept, segs, rec);
}

}  // namespace nhans
