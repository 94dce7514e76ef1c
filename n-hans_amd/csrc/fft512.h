// The 512-point transform of stoi.hip and quality.hip as one thread sees it: 512 = 8 x 8 x 8, three Stockham stages of
// radix 8 on 64 threads, eight complex doubles per thread in registers and two exchanges through a buffer between the
// stages.  The per-lane steps are plain functions of the thread's index j, so that a host program can run the 64 "threads"
// of a stage in a loop and hold the result to a direct transform; what a kernel adds to them -- the barriers between the
// stages -- is at the end, beside the host's twiddle table.
//
// Stage with sub-transform length NS (1, 8, 64), thread j, k = j mod NS:
//     v[r] = in[j + 64 r] * W^(r k 512 / (8 NS)),  W = exp(-2 pi i / 512);   V = DFT8(v);
//     out[(j - k) * 8 + k + r NS] = V[r];          after the third stage out is the transform in natural order, and thread
//     j holds bins j + 64 r in V[r] without storing them.
// The buffer is two arrays of doubles (real, imaginary) indexed through fft512_pad: one spare double after every eight, so
// that the stores of the first stage -- thread j at 8 j + r -- fall 9 doubles apart and spread over all banks where a
// stride of 8 doubles would put 32 lanes on four of them (a bank is 4 bytes; an 8-byte access of 32 lanes takes two
// passes at best, and takes two with this stride).  The loads of every stage -- thread j at j + 64 r -- are consecutive
// but for the spare ones.
// The complex arithmetic is written with plain *, + and -: how the compiler contracts them is part of the result.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FFT512_HD __host__ __device__ __forceinline__
#else
#define FFT512_HD inline
#endif

namespace nhans {

constexpr int kFft512Buf = 512 + 512 / 8;       // doubles per array of the exchange buffer

FFT512_HD int fft512_pad(int p) { return p + (p >> 3); }

struct Fft512C {
    double r, i;
};
FFT512_HD Fft512C fft512_add(Fft512C a, Fft512C b) { return {a.r + b.r, a.i + b.i}; }
FFT512_HD Fft512C fft512_sub(Fft512C a, Fft512C b) { return {a.r - b.r, a.i - b.i}; }
FFT512_HD Fft512C fft512_mul(Fft512C a, double c, double s) { return {a.r * c - a.i * s, a.r * s + a.i * c}; }     // a (c + i s)
FFT512_HD Fft512C fft512_mul_neg_i(Fft512C a) { return {a.i, -a.r}; }

// y0 .. y3 = the 4-point transform of c0 .. c3
FFT512_HD void fft512_dft4(Fft512C c0, Fft512C c1, Fft512C c2, Fft512C c3, Fft512C& y0, Fft512C& y1, Fft512C& y2, Fft512C& y3) {
    const Fft512C p0 = fft512_add(c0, c2), p1 = fft512_sub(c0, c2), q0 = fft512_add(c1, c3), q1 = fft512_mul_neg_i(fft512_sub(c1, c3));
    y0 = fft512_add(p0, q0); y2 = fft512_sub(p0, q0);
    y1 = fft512_add(p1, q1); y3 = fft512_sub(p1, q1);
}

// v <- the 8-point transform of v, in natural order (decimation in frequency: the even bins are the 4-point transform of
// the sums, the odd ones that of the differences times W8^i)
FFT512_HD void fft512_dft8(Fft512C* v) {
    const double h = 0.70710678118654752440;
    const Fft512C a0 = fft512_add(v[0], v[4]), a1 = fft512_add(v[1], v[5]), a2 = fft512_add(v[2], v[6]), a3 = fft512_add(v[3], v[7]);
    const Fft512C b0 = fft512_sub(v[0], v[4]), d1 = fft512_sub(v[1], v[5]), d2 = fft512_sub(v[2], v[6]), d3 = fft512_sub(v[3], v[7]);
    const Fft512C b1 = {(d1.r + d1.i) * h, (d1.i - d1.r) * h};          // times (1 - i) / sqrt 2
    const Fft512C b2 = fft512_mul_neg_i(d2);
    const Fft512C b3 = {(d3.i - d3.r) * h, (-d3.r - d3.i) * h};         // times (-1 - i) / sqrt 2
    fft512_dft4(a0, a1, a2, a3, v[0], v[2], v[4], v[6]);
    fft512_dft4(b0, b1, b2, b3, v[1], v[3], v[5], v[7]);
}

// v[r] <- in[j + 64 r]
FFT512_HD void fft512_load(int j, const double* re, const double* im, Fft512C* v) {
    for (int r = 0; r < 8; ++r) {
        const int p = fft512_pad(j + 64 * r);
        v[r] = {re[p], im[p]};
    }
}

// the twiddles of a stage with sub-transform length NS (tw_c / tw_s: cos and -sin of 2 pi t / 512, t < 512), then DFT8
template <int NS>
FFT512_HD void fft512_butterfly(int j, const double* tw_c, const double* tw_s, Fft512C* v) {
    if (NS > 1) {
        const int k = j & (NS - 1);
        for (int r = 1; r < 8; ++r) {
            const int t = r * k * (512 / (8 * NS));
            v[r] = fft512_mul(v[r], tw_c[t], tw_s[t]);
        }
    }
    fft512_dft8(v);
}

// out[(j - k) * 8 + k + r NS] <- v[r]
template <int NS>
FFT512_HD void fft512_store(int j, const Fft512C* v, double* re, double* im) {
    const int k = j & (NS - 1);
    for (int r = 0; r < 8; ++r) {
        const int p = fft512_pad((j - k) * 8 + k + r * NS);
        re[p] = v[r].r; im[p] = v[r].i;
    }
}

// (host) the twiddle table: cos of 2 pi t / 512 for t < 512, then -sin
inline void fft512_twiddles(double* cos_then_neg_sin) {
    const double pi = 3.14159265358979323846;
    for (int t = 0; t < 512; ++t) {
        const double a = 2.0 * pi * (double)t / 512.0;
        cos_then_neg_sin[t] = std::cos(a);
        cos_then_neg_sin[512 + t] = -std::sin(a);
    }
}

#if defined(__HIPCC__)
// The transform of one wavefront's frame: thread j = lane brings samples j + 64 r in v[r] and leaves with bins j + 64 r
// there; tc / ts are the table of fft512_twiddles in LDS, re / im the wavefront's own exchange buffer (kFft512Buf doubles
// each).  There are four workgroup barriers inside, so EVERY thread of the workgroup must call it: a wavefront without
// a frame runs it on zeros.  A kernel that has just copied the twiddles into LDS needs no barrier of its own before the
// call: the first stage reads none, and the first barrier here publishes them.
__device__ __forceinline__ void fft512_wave(int j, const double* tc, const double* ts, Fft512C* v, double* re, double* im) {
    fft512_butterfly<1>(j, tc, ts, v);
    fft512_store<1>(j, v, re, im);
    __syncthreads();
    fft512_load(j, re, im, v);
    __syncthreads();
    fft512_butterfly<8>(j, tc, ts, v);
    fft512_store<8>(j, v, re, im);
    __syncthreads();
    fft512_load(j, re, im, v);
    __syncthreads();
    fft512_butterfly<64>(j, tc, ts, v);
}
#endif

}  // namespace nhans
