// The 512-point transform of stoi.hip as one thread sees it: 512 = 8 x 8 x 8, three Stockham stages of radix 8 on 64
// threads, eight complex doubles per thread in registers and two exchanges through a buffer between the stages.  Plain
// functions of the thread's index j, so that a host program can run the 64 "threads" of a stage in a loop and hold the
// result to a direct transform.
//
// Stage with sub-transform length NS (1, 8, 64), thread j, k = j mod NS:
//     v[r] = in[j + 64 r] * W^(r k 512 / (8 NS)),  W = exp(-2 pi i / 512);   V = DFT8(v);
//     out[(j - k) * 8 + k + r NS] = V[r];          after the third stage out is the transform in natural order, and thread
//     j holds bins j + 64 r in V[r] without storing them.
// The buffer is two arrays of doubles (real, imaginary) indexed through stoi_pad: one spare double after every eight, so
// that the stores of the first stage -- thread j at 8 j + r -- fall 9 doubles apart and spread over all banks where a
// stride of 8 doubles would put 32 lanes on four of them (a bank is 4 bytes; an 8-byte access of 32 lanes takes two
// passes at best, and takes two with this stride).  The loads of every stage -- thread j at j + 64 r -- are consecutive
// but for the spare ones.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STOI_HD __host__ __device__ __forceinline__
#else
#define STOI_HD inline
#endif

namespace nhans {

constexpr int kStoiFftBuf = 512 + 512 / 8;      // doubles per array of the exchange buffer

STOI_HD int stoi_pad(int p) { return p + (p >> 3); }

struct StoiC {
    double r, i;
};
STOI_HD StoiC stoi_add(StoiC a, StoiC b) { return {a.r + b.r, a.i + b.i}; }
STOI_HD StoiC stoi_sub(StoiC a, StoiC b) { return {a.r - b.r, a.i - b.i}; }
STOI_HD StoiC stoi_mul(StoiC a, double c, double s) { return {a.r * c - a.i * s, a.r * s + a.i * c}; }     // a (c + i s)
STOI_HD StoiC stoi_mul_neg_i(StoiC a) { return {a.i, -a.r}; }

// y0 .. y3 = the 4-point transform of c0 .. c3
STOI_HD void stoi_dft4(StoiC c0, StoiC c1, StoiC c2, StoiC c3, StoiC& y0, StoiC& y1, StoiC& y2, StoiC& y3) {
    const StoiC p0 = stoi_add(c0, c2), p1 = stoi_sub(c0, c2), q0 = stoi_add(c1, c3), q1 = stoi_mul_neg_i(stoi_sub(c1, c3));
    y0 = stoi_add(p0, q0); y2 = stoi_sub(p0, q0);
    y1 = stoi_add(p1, q1); y3 = stoi_sub(p1, q1);
}

// v <- the 8-point transform of v, in natural order (decimation in frequency: the even bins are the 4-point transform of
// the sums, the odd ones that of the differences times W8^i)
STOI_HD void stoi_dft8(StoiC* v) {
    const double h = 0.70710678118654752440;
    const StoiC a0 = stoi_add(v[0], v[4]), a1 = stoi_add(v[1], v[5]), a2 = stoi_add(v[2], v[6]), a3 = stoi_add(v[3], v[7]);
    const StoiC b0 = stoi_sub(v[0], v[4]), d1 = stoi_sub(v[1], v[5]), d2 = stoi_sub(v[2], v[6]), d3 = stoi_sub(v[3], v[7]);
    const StoiC b1 = {(d1.r + d1.i) * h, (d1.i - d1.r) * h};            // times (1 - i) / sqrt 2
    const StoiC b2 = stoi_mul_neg_i(d2);
    const StoiC b3 = {(d3.i - d3.r) * h, (-d3.r - d3.i) * h};           // times (-1 - i) / sqrt 2
    stoi_dft4(a0, a1, a2, a3, v[0], v[2], v[4], v[6]);
    stoi_dft4(b0, b1, b2, b3, v[1], v[3], v[5], v[7]);
}

// v[r] <- in[j + 64 r]
STOI_HD void stoi_fft_load(int j, const double* re, const double* im, StoiC* v) {
    for (int r = 0; r < 8; ++r) {
        const int p = stoi_pad(j + 64 * r);
        v[r] = {re[p], im[p]};
    }
}

// the twiddles of a stage with sub-transform length NS (tw_c / tw_s: cos and -sin of 2 pi t / 512, t < 512), then DFT8
template <int NS>
STOI_HD void stoi_fft_butterfly(int j, const double* tw_c, const double* tw_s, StoiC* v) {
    if (NS > 1) {
        const int k = j & (NS - 1);
        for (int r = 1; r < 8; ++r) {
            const int t = r * k * (512 / (8 * NS));
            v[r] = stoi_mul(v[r], tw_c[t], tw_s[t]);
        }
    }
    stoi_dft8(v);
}

// out[(j - k) * 8 + k + r NS] <- v[r]
template <int NS>
STOI_HD void stoi_fft_store(int j, const StoiC* v, double* re, double* im) {
    const int k = j & (NS - 1);
    for (int r = 0; r < 8; ++r) {
        const int p = stoi_pad((j - k) * 8 + k + r * NS);
        re[p] = v[r].r; im[p] = v[r].i;
    }
}

}  // namespace nhans
