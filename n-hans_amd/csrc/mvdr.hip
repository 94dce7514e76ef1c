// Mask-driven MVDR beamforming (include/nhans_hip.h: nhans_mvdr_*).
//
//   mvdr_spectra_kernel : the C planes of every clip -> complex spectra X_c[t, k]: stft_features_kernel's forward transform
//                         (fft400.h, stft_common.h) with a complex store; the analysis rows on request
//   mvdr_cov_kernel<C>  : the masked covariances of every (clip, bin) in double, and the bin's sum |X_r|^2
//   mvdr_solve_kernel<C>: per (clip, bin) the loading, the Cholesky factor, C pairs of triangular solves, w; the clip's
//                         fallback count and energy_ref
//   mvdr_apply_kernel<C>: y = w^H x in double, rounded once to complex float32, as rows; a frame's sum |y|^2
//   mvdr_energy_kernel  : a clip's energy_out from the frame sums
//
// A channel-clip (clip i, channel c) is a clip of its own to the transform: its samples begin at C off[i] + c n_i and its
// T_i rows at C foff[i] + c T_i, so the planes and X have one layout and the C n_i samples of a clip are C whole clips
// one after the other.
// Covariance: the bin is on the lane (a row of X_c is read coalesced) and the ENTRIES are split over the four waves of a
// workgroup, not the frames: wave w owns the upper-triangle entries e = w, w + 4, ... of both matrices -- at C = 8 nine of
// the 36, 36 doubles per lane -- and walks the clip's frames once, in ascending order.  Every entry has one owner, so there
// is no reduction through LDS and the order of the sum is the plainest one there is; the price is that the four waves
// read the same C values of X (the second to fourth reads hit the cache) and that a clip's frames are a serial chain.
// Solve: one lane per (clip, bin); the factor lives in registers (C <= 8: 36 complex doubles), the columns of Phi_s pass
// through one at a time.
#include "stft_common.h"
#include "score_common.h"

#include <type_traits>

namespace nhans {

// ---------------------------------------------------------------------------------------------
// stft_features_kernel's run walk and transform (stft.hip, where the design is described) around the same fft400.h passes,
// with a complex store.  It is restated here, as phase.hip restates it, and not shared as one templated body: a body
// shared through stft_common.h was built, and the compiler then contracts two products of the transform differently in
// stft_features_kernel itself, whose rows changed in their last bits on the device.  The existing kernel stays as it is;
// tests/test_gpu_mvdr.py holds the rows of the two kernels to each other bit for bit.
__global__ void __launch_bounds__(256) mvdr_spectra_kernel(
    const float* __restrict__ wav, ClipTable tab, const int* __restrict__ block_clip, const int* __restrict__ block_f0, int nblocks,
    const cplx* __restrict__ tw400g, const float* __restrict__ windowg, cplx* __restrict__ X, float* __restrict__ logmag,
    float* __restrict__ phase) {
    constexpr int F = kStftFramesPerBlock;
    constexpr int SPAN = kWin + kHop * (F - 1);
    __shared__ __attribute__((aligned(16))) float xs[SPAN];
    __shared__ float win[kWin];
    __shared__ cplx tw[400];
    __shared__ cplx tbuf[F * kTReal];              // T[frame][k1][n2], rows padded to 21

    const int tid = threadIdx.x;
    constexpr int NPRE = (SPAN + 255) / 256;        // samples per thread of one run
    float pre[NPRE];
    auto fetch = [&](int blk) {                     // the run's samples -> registers (loads stay in flight)
        const int c = block_clip[blk];
        const int64_t base = tab.sample_off[c] + (int64_t)block_f0[blk] * kHop;
        const int left = (int)min((int64_t)SPAN, tab.sample_off[c + 1] - base);      // samples of the run inside the clip
        const float* __restrict__ wb = wav + base;                                   // uniform base + 32-bit lane offset
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int i = u * 256 + tid;
            pre[u] = i < left ? ldg32(wb, (unsigned)i * 4u) : 0.f;
        }
    };
    for (int i = tid; i < 400; i += 256) { tw[i] = tw400g[i]; win[i] = windowg[i]; }
    fetch(blockIdx.x);

#pragma unroll 1
  for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int clip = block_clip[blk], f0 = block_f0[blk];
    const int64_t fr_beg = tab.frame_off[clip];
    const int T = (int)(tab.frame_off[clip + 1] - fr_beg);
#pragma unroll
    for (int u = 0; u < NPRE; ++u) {
        const int i = u * 256 + tid;
        if (i < SPAN) xs[i] = pre[u];
    }
    __syncthreads();                                // (also: every lane is through with the previous run's rows)
    if (blk + (int)gridDim.x < nblocks) fetch(blk + gridDim.x);

    // pass 1: task (frame f, column n2) = real 20-point DFT over n1 of the windowed samples x[20*n1 + n2]
#pragma unroll 1
    for (int id = tid; id < F * 20; id += 256) {
        const int f = id / 20, n2 = id - f * 20;
        float col[20];
        cplx y[kRows];
        const float* xf = xs + f * kHop + n2;
#pragma unroll
        for (int n1 = 0; n1 < 20; ++n1) col[n1] = xf[20 * n1] * win[20 * n1 + n2];
        fft400_pass1_real(col, n2, tw, y);
        cplx* tf = tbuf + f * kTReal + n2;
#pragma unroll
        for (int k1 = 0; k1 < kRows; ++k1) tf[k1 * kTRow] = y[k1];
    }
    __syncthreads();
    // pass 2: task (frame f, row k1 <= 10) = complex 20-point DFT over n2 -> X[k1 + 20*k2], k2 = 0..19
    if (tid < F * kRows) {
        const int f = tid / kRows, k1 = tid - f * kRows;
        cplx row[20], X20[20];
        const cplx* tf = tbuf + f * kTReal + k1 * kTRow;
#pragma unroll
        for (int n2 = 0; n2 < 20; ++n2) row[n2] = tf[n2];
        fft400_pass2<false>(row, X20);
        if (f0 + f < T) {
            cplx* __restrict__ xo = X + (fr_beg + f0 + f) * kBins;                 // the frame's row (64-bit once per lane)
            float* __restrict__ lo_ = logmag ? logmag + (fr_beg + f0 + f) * kBins : nullptr;
            float* __restrict__ po_ = phase ? phase + (fr_beg + f0 + f) * kBins : nullptr;
            // k2 < 10: bin k1 + 20*k2 as computed.  k2 >= 10: bin 400 - (k1 + 20*k2) as the conjugate (rows 1..9);
            // row 0 has the Nyquist bin 200 at k2 = 10 and nothing else there, row 10 nothing.
#pragma unroll
            for (int k2 = 0; k2 < 20; ++k2) {
                const bool mirror = k2 >= 10 && k1 != 0;
                const bool live = k2 < 10 || (k1 == 0 ? k2 == 10 : k1 != 10);
                if (!live) continue;
                const int bin = mirror ? 400 - k1 - 20 * k2 : k1 + 20 * k2;
                const cplx v = X20[k2];
                xo[bin] = cmake(v.x, mirror ? -v.y : v.y);
                // (the analysis kernel's two functions of the same registers: nhans_stft_features' rows)
                if (lo_) lo_[bin] = fast_log(__builtin_amdgcn_sqrtf(v.x * v.x + v.y * v.y) + 1e-5f);
                if (po_) po_[bin] = fast_atan2(mirror ? -v.y : v.y, v.x);
            }
        }
    }
  }
}

void launch_mvdr_spectra(const float* wav, ClipTable t, const int* block_clip, const int* block_f0, int nblocks, const float* tw400,
                         const float* window, float* X, float* logmag, float* phase, hipStream_t s) {
    if (nblocks <= 0) return;
    const int grid = nblocks < 256 * 2 ? nblocks : 256 * 2;             // two resident workgroups per CU, as launch_stft
    NHANS_LAUNCH("mvdr_spectra", mvdr_spectra_kernel, dim3(grid), dim3(256), 0, s, wav, t, block_clip, block_f0, nblocks,
                 reinterpret_cast<const cplx*>(tw400), window, reinterpret_cast<cplx*>(X), logmag, phase);
}

// ---------------------------------------------------------------------------------------------
// m of a mask row's value: min(max(v, 0), 1) with max(NaN, 0) = 0 -- a NaN counts as 0; a log-gain goes through
// nhans_istft's exp first
__device__ __forceinline__ float mvdr_mask(float v, int flags) {
    if (flags & kMvdrLogGain) v = v > 0.f ? 1.f : fast_exp(v);       // min(1, exp(g)) without the overflow
    return fminf(fmaxf(v, 0.f), 1.f);
}

// entry e of the upper triangle, rows ascending: (0,0) (0,1) ... (0,C-1) (1,1) ...
template <int C> constexpr int tri_row(int e) {
    int i = 0;
    while (e >= C - i) { e -= C - i; ++i; }
    return i;
}
template <int C> constexpr int tri_col(int e) {
    int i = 0;
    while (e >= C - i) { e -= C - i; ++i; }
    return i + e;
}

// f(integral_constant 0), ..., f(integral_constant N - 1): a loop whose index is a constant expression in its body
template <int N, typename F> __device__ __forceinline__ void static_for(F f) {
    if constexpr (N > 0) { static_for<N - 1>(f); f(std::integral_constant<int, N - 1>{}); }
}

// One workgroup: (clip, group of 64 bins); wave W: the entries e = W, W + 4, ...
template <int C, int W>
__device__ __forceinline__ void mvdr_cov_wave(const cplx* __restrict__ Xc, const float* __restrict__ mrow, int T, int bin, bool live, int flags,
                                              int ref, double2* __restrict__ phi, double* __restrict__ eref) {
    constexpr int NE = C * (C + 1) / 2;
    constexpr int N = NE > W ? (NE - W + 3) / 4 : 0;
    double sr[N > 0 ? N : 1], si[N > 0 ? N : 1], nr[N > 0 ? N : 1], ni[N > 0 ? N : 1];
#pragma unroll
    for (int a = 0; a < (N > 0 ? N : 1); ++a) { sr[a] = si[a] = nr[a] = ni[a] = 0.0; }
    double er = 0.0;
    const size_t plane = (size_t)T * kBins;              // one channel of the clip
    cplx x[C], xn[C];
    float mv = 0.f, mn = 0.f;
    if (N > 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) xn[c] = Xc[c * plane + bin];
        mn = mrow[bin];
#pragma unroll 1
        for (int t = 0; t < T; ++t) {
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = xn[c];
            mv = mn;
            if (t + 1 < T) {                              // the next frame's values are on their way under this frame's sums
                const size_t o = (size_t)(t + 1) * kBins + bin;
#pragma unroll
                for (int c = 0; c < C; ++c) xn[c] = Xc[c * plane + o];
                mn = mrow[o];
            }
            const double md = (double)mvdr_mask(mv, flags);
            const double nd = 1.0 - md;
            static_for<N>([&](auto a_) {
                constexpr int a = decltype(a_)::value, e = W + 4 * a;
                constexpr int i = tri_row<C>(e), j = tri_col<C>(e);
                const double ar = (double)x[i].x, ai = (double)x[i].y, br = (double)x[j].x, bi = (double)x[j].y;
                // x_i conj(x_j): two products of float32 are exact in double, so each part is rounded once
                const double pr = fma(ar, br, ai * bi);
                sr[a] = fma(md, pr, sr[a]);
                nr[a] = fma(nd, pr, nr[a]);
                if (i != j) {
                    const double pi = fma(ai, br, -(ar * bi));
                    si[a] = fma(md, pi, si[a]);
                    ni[a] = fma(nd, pi, ni[a]);
                }
            });
            if (W == 0) {
                cplx xr = x[0];
#pragma unroll
                for (int c = 1; c < C; ++c) xr = ref == c ? x[c] : xr;
                const double ar = (double)xr.x, ai = (double)xr.y;
                er += fma(ar, ar, ai * ai);
            }
        }
    }
    if (!live) return;
    // [which][i][j][bin], both triangles
    static_for<N>([&](auto a_) {
        constexpr int a = decltype(a_)::value, e = W + 4 * a;
        constexpr int i = tri_row<C>(e), j = tri_col<C>(e);
        double2* ps = phi + ((size_t)(0 * C + i) * C + j) * kBins + bin;
        double2* pn = phi + ((size_t)(1 * C + i) * C + j) * kBins + bin;
        *ps = make_double2(sr[a], i == j ? 0.0 : si[a]);
        *pn = make_double2(nr[a], i == j ? 0.0 : ni[a]);
        if (i != j) {
            phi[((size_t)(0 * C + j) * C + i) * kBins + bin] = make_double2(sr[a], -si[a]);
            phi[((size_t)(1 * C + j) * C + i) * kBins + bin] = make_double2(nr[a], -ni[a]);
        }
    });
    if (W == 0) eref[bin] = er;
}

template <int C>
__global__ void __launch_bounds__(256) mvdr_cov_kernel(const cplx* __restrict__ X, const float* __restrict__ mask,
                                                       const int64_t* __restrict__ frame_off, int flags, int ref,
                                                       double2* __restrict__ phi, double* __restrict__ eref) {
    const int clip = blockIdx.x >> 2, group = blockIdx.x & 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t fb = frame_off[clip];
    const int T = (int)(frame_off[clip + 1] - fb);
    const int k = group * 64 + lane;
    const bool live = k < kBins;
    const int bin = live ? k : kBins - 1;               // (a lane past the last bin reads the last bin and stores nothing)
    const cplx* Xc = X + (size_t)C * fb * kBins;
    const float* mrow = mask + (size_t)fb * kBins;
    double2* ph = phi + (size_t)clip * 2 * C * C * kBins;
    double* er = eref + (size_t)clip * kBins;
    switch (wave) {                                     // (wave-uniform)
    case 0: mvdr_cov_wave<C, 0>(Xc, mrow, T, bin, live, flags, ref, ph, er); break;
    case 1: mvdr_cov_wave<C, 1>(Xc, mrow, T, bin, live, flags, ref, ph, er); break;
    case 2: mvdr_cov_wave<C, 2>(Xc, mrow, T, bin, live, flags, ref, ph, er); break;
    default: mvdr_cov_wave<C, 3>(Xc, mrow, T, bin, live, flags, ref, ph, er); break;
    }
}

// ---------------------------------------------------------------------------------------------
// One workgroup per clip, lane k < 201: bin k.
template <int C>
__global__ void __launch_bounds__(256) mvdr_solve_kernel(const double2* __restrict__ phi, const double* __restrict__ eref,
                                                         const int64_t* __restrict__ frame_off, int ref, double loading,
                                                         double2* __restrict__ w_out, double* __restrict__ rec_out) {
    __shared__ double es[256];
    __shared__ int fbs[4];
    const int clip = blockIdx.x, k = threadIdx.x;
    const bool live = k < kBins;
    const int bin = live ? k : kBins - 1;
    const double2* ps = phi + (size_t)clip * 2 * C * C * kBins + bin;
    const double2* pn = ps + (size_t)C * C * kBins;
    auto at = [&](const double2* p, int i, int j) { return p[(size_t)(i * C + j) * kBins]; };

    // the lower triangle of Phi_n, its trace (diagonal ascending) and the loading
    double Lr[C][C], Li[C][C];
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) { const double2 v = at(pn, i, j); Lr[i][j] = v.x; Li[i][j] = v.y; }
        tr += Lr[i][i];
    }
    bool ok = tr != 0.0;                                // (a NaN trace passes here and fails its first pivot)
    const double add = loading * (tr / (double)C);
#pragma unroll
    for (int i = 0; i < C; ++i) Lr[i][i] += add;
    // Cholesky, column by column: Phi_n' = L L^H, the diagonal of L real
#pragma unroll
    for (int j = 0; j < C; ++j) {
        double d = Lr[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) { d = fma(-Lr[j][q], Lr[j][q], d); d = fma(-Li[j][q], Li[j][q], d); }
        ok = ok && d > 0.0 && d < __longlong_as_double(0x7ff0000000000000LL);
        const double ljj = sqrt(d);
        Lr[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < C; ++i) {
            double sr = Lr[i][j], si = Li[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) {               // - L[i][q] conj(L[j][q])
                sr = fma(-Lr[i][q], Lr[j][q], sr); sr = fma(-Li[i][q], Li[j][q], sr);
                si = fma(-Li[i][q], Lr[j][q], si); si = fma(Lr[i][q], Li[j][q], si);
            }
            Lr[i][j] = sr / ljj; Li[i][j] = si / ljj;
        }
    }
    // G = Phi_n'^-1 Phi_s, a column at a time: tau = sum Re G[j][j] (j ascending), column ref is kept
    double tau = 0.0, wr[C], wi[C];
#pragma unroll
    for (int i = 0; i < C; ++i) { wr[i] = 0.0; wi[i] = 0.0; }
#pragma unroll
    for (int col = 0; col < C; ++col) {
        double gr[C], gi[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {                   // L y = b
            const double2 b = at(ps, i, col);
            double sr = b.x, si = b.y;
#pragma unroll
            for (int q = 0; q < i; ++q) {               // - L[i][q] y[q]
                sr = fma(-Lr[i][q], gr[q], sr); sr = fma(Li[i][q], gi[q], sr);
                si = fma(-Lr[i][q], gi[q], si); si = fma(-Li[i][q], gr[q], si);
            }
            gr[i] = sr / Lr[i][i]; gi[i] = si / Lr[i][i];
        }
#pragma unroll
        for (int i = C - 1; i >= 0; --i) {              // L^H g = y
            double sr = gr[i], si = gi[i];
#pragma unroll
            for (int q = C - 1; q > i; --q) {           // - conj(L[q][i]) g[q]
                sr = fma(-Lr[q][i], gr[q], sr); sr = fma(-Li[q][i], gi[q], sr);
                si = fma(-Lr[q][i], gi[q], si); si = fma(Li[q][i], gr[q], si);
            }
            gr[i] = sr / Lr[i][i]; gi[i] = si / Lr[i][i];
        }
        tau += gr[col];
        if (col == ref) {
#pragma unroll
            for (int i = 0; i < C; ++i) { wr[i] = gr[i]; wi[i] = gi[i]; }
        }
    }
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    ok = ok && tau > 0.0 && tau < inf;
#pragma unroll
    for (int i = 0; i < C; ++i) {
        wr[i] = wr[i] / tau; wi[i] = wi[i] / tau;
        ok = ok && fabs(wr[i]) < inf && fabs(wi[i]) < inf;
    }
    if (live) {
        double2* wo = w_out + ((size_t)clip * kBins + bin) * C;
#pragma unroll
        for (int i = 0; i < C; ++i) wo[i] = ok ? make_double2(wr[i], wi[i]) : make_double2(i == ref ? 1.0 : 0.0, 0.0);
    }
    if (!rec_out) return;
    // the record: the bins that fell back (a count) and energy_ref = the bins' sums, lane l of 64 summing bins l, l + 64,
    // l + 128, l + 192 ascending, the 64 sums by wave_sum
    es[k] = live ? eref[(size_t)clip * kBins + bin] : 0.0;
    const unsigned long long fbm = __ballot(live && !ok);
    if ((k & 63) == 0) fbs[k >> 6] = __popcll(fbm);
    __syncthreads();
    if (k < 64) {
        double e = es[k];
        e = __dadd_rn(e, es[k + 64]); e = __dadd_rn(e, es[k + 128]); e = __dadd_rn(e, es[k + 192]);
        e = wave_sum(e);
        if (k == 0) {
            double* r = rec_out + (size_t)clip * kMvdrFields;
            r[0] = (double)(frame_off[clip + 1] - frame_off[clip]);
            r[1] = (double)C;
            r[2] = (double)ref;
            r[3] = (double)(fbs[0] + fbs[1] + fbs[2] + fbs[3]);
            r[4] = e;
            r[5] = quiet_nan();                         // energy_out: the filter's to write
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One workgroup: a run of kMvdrRun frames of a clip; wave v takes frames f0 + v, f0 + v + 4, ...; lane l the bins l,
// l + 64, l + 128 and (l < 9) l + 192, one after the other: a bin's weights stay in registers over the wave's frames.
template <int C>
__global__ void __launch_bounds__(256) mvdr_apply_kernel(const cplx* __restrict__ X, const double2* __restrict__ w,
                                                         const float* __restrict__ gain, const int64_t* __restrict__ frame_off,
                                                         const int* __restrict__ block_clip, const int* __restrict__ block_f0,
                                                         float* __restrict__ logmag, float* __restrict__ phase,
                                                         cplx* __restrict__ yout, double* __restrict__ eframe) {
    const int clip = block_clip[blockIdx.x], f0 = block_f0[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t fb = frame_off[clip];
    const int T = (int)(frame_off[clip + 1] - fb);
    const int f1 = f0 + kMvdrRun < T ? f0 + kMvdrRun : T;
    const size_t plane = (size_t)T * kBins;
    const cplx* Xc = X + (size_t)C * fb * kBins;
    const int nslot = lane < kBins - 192 ? 4 : 3;
    constexpr int NF = kMvdrRun / 4;                    // frames of a wave
    double e[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) e[j] = 0.0;
#pragma unroll 1
    for (int u = 0; u < 4; ++u) {                       // a lane's bins ascending: a frame's sum takes them in this order
        if (u >= nslot) break;
        const int bin = lane + 64 * u;
        double wr[C], wi[C];
        const double2* wb = w + ((size_t)clip * kBins + bin) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) { const double2 v = wb[c]; wr[c] = v.x; wi[c] = v.y; }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int t = f0 + wave + 4 * j;
            if (t < f1) {                               // (wave-uniform)
                const size_t row = (size_t)(fb + t) * kBins;
                double yr = 0.0, yi = 0.0;
#pragma unroll
                for (int c = 0; c < C; ++c) {           // conj(w_c) x_c, channels ascending
                    const cplx x = Xc[c * plane + (size_t)t * kBins + bin];
                    const double xr = (double)x.x, xi = (double)x.y;
                    yr = fma(wr[c], xr, yr); yr = fma(wi[c], xi, yr);
                    yi = fma(wr[c], xi, yi); yi = fma(-wi[c], xr, yi);
                }
                const float re = (float)yr, im = (float)yi;         // the one rounding to float32
                if (yout) yout[row + bin] = cmake(re, im);
                float lm = fast_log(fmaxf(__builtin_amdgcn_sqrtf(re * re + im * im), 1e-5f));
                if (gain) lm += gain[row + bin];
                logmag[row + bin] = lm;
                phase[row + bin] = fast_atan2(im, re);
                e[j] = fma((double)re, (double)re, e[j]); e[j] = fma((double)im, (double)im, e[j]);
            }
        }
    }
    if (eframe) {                                       // a frame's sum |y|^2: the lane's bins ascending, then the tree
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int t = f0 + wave + 4 * j;
            if (t < f1) {
                const double s = wave_sum(e[j]);
                if (lane == 0) eframe[fb + t] = s;
            }
        }
    }
}

// One wavefront per clip: lane l sums frames l, l + 64, ... ascending, the 64 sums by wave_sum -> field 5 of the record.
__global__ void __launch_bounds__(64) mvdr_energy_kernel(const double* __restrict__ eframe, const int64_t* __restrict__ frame_off,
                                                         double* __restrict__ rec) {
    const int clip = blockIdx.x;
    const int64_t b = frame_off[clip], e = frame_off[clip + 1];
    double s = 0.0;
    for (int64_t f = b + threadIdx.x; f < e; f += 64) s = __dadd_rn(s, eframe[f]);
    s = wave_sum(s);
    if (threadIdx.x == 0) rec[(size_t)clip * kMvdrFields + 5] = s;
}

// ---------------------------------------------------------------------------------------------
template <int C>
static void weights_launch(const float* X, const float* mask, const int64_t* frame_off_dev, int nclips, int ref, double loading,
                           int flags, double* phi, double* eref, double* w_out, double* rec_out, bool solve, hipStream_t s) {
    if (!solve)
        NHANS_LAUNCH("mvdr_cov", mvdr_cov_kernel<C>, dim3(4 * nclips), dim3(256), 0, s, reinterpret_cast<const cplx*>(X), mask,
                     frame_off_dev, flags, ref, reinterpret_cast<double2*>(phi), eref);
    else
        NHANS_LAUNCH("mvdr_solve", mvdr_solve_kernel<C>, dim3(nclips), dim3(256), 0, s, reinterpret_cast<const double2*>(phi), eref,
                     frame_off_dev, ref, loading, reinterpret_cast<double2*>(w_out), rec_out);
}

static void weights_dispatch(const float* X, const float* mask, const int64_t* frame_off_dev, int nclips, int C, int ref, double loading,
                             int flags, double* phi, double* eref, double* w_out, double* rec_out, bool solve, hipStream_t s) {
    if (!tiles_ok(solve ? "mvdr_solve" : "mvdr_cov", nclips, solve ? (long long)nclips : 4LL * nclips)) return;
    switch (C) {
    case 1: weights_launch<1>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 2: weights_launch<2>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 3: weights_launch<3>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 4: weights_launch<4>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 5: weights_launch<5>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 6: weights_launch<6>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 7: weights_launch<7>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    case 8: weights_launch<8>(X, mask, frame_off_dev, nclips, ref, loading, flags, phi, eref, w_out, rec_out, solve, s); break;
    default: note_refusal(solve ? "mvdr_solve" : "mvdr_cov");
    }
}

void launch_mvdr_cov(const float* X, const float* mask, const int64_t* frame_off_dev, int nclips, int C, int ref, int flags, double* phi,
                     double* eref, hipStream_t s) {
    weights_dispatch(X, mask, frame_off_dev, nclips, C, ref, 0.0, flags, phi, eref, nullptr, nullptr, false, s);
}

void launch_mvdr_solve(const double* phi, const double* eref, const int64_t* frame_off_dev, int nclips, int C, int ref, double loading,
                       double* w_out, double* rec_out, hipStream_t s) {
    weights_dispatch(nullptr, nullptr, frame_off_dev, nclips, C, ref, loading, 0, const_cast<double*>(phi), const_cast<double*>(eref), w_out,
                     rec_out, true, s);
}

template <int C>
static void apply_launch(const float* X, const double* w, const float* gain, const int64_t* frame_off_dev, const int* block_clip,
                         const int* block_f0, int nblocks, float* logmag, float* phase, float* y, double* eframe, hipStream_t s) {
    NHANS_LAUNCH("mvdr_apply", mvdr_apply_kernel<C>, dim3(nblocks), dim3(256), 0, s, reinterpret_cast<const cplx*>(X),
                 reinterpret_cast<const double2*>(w), gain, frame_off_dev, block_clip, block_f0, logmag, phase,
                 reinterpret_cast<cplx*>(y), eframe);
}

void launch_mvdr_apply(const float* X, const double* w, const float* gain, const int64_t* frame_off_dev, const int* block_clip,
                       const int* block_f0, int nblocks, int C, float* logmag, float* phase, float* y, double* eframe, hipStream_t s) {
    if (!tiles_ok("mvdr_apply", 1, nblocks)) return;
    switch (C) {
    case 1: apply_launch<1>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 2: apply_launch<2>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 3: apply_launch<3>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 4: apply_launch<4>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 5: apply_launch<5>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 6: apply_launch<6>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 7: apply_launch<7>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    case 8: apply_launch<8>(X, w, gain, frame_off_dev, block_clip, block_f0, nblocks, logmag, phase, y, eframe, s); break;
    default: note_refusal("mvdr_apply");
    }
}

void launch_mvdr_energy(const double* eframe, const int64_t* frame_off_dev, int nclips, double* rec, hipStream_t s) {
    if (!tiles_ok("mvdr_energy", nclips, nclips)) return;
    NHANS_LAUNCH("mvdr_energy", mvdr_energy_kernel, dim3(nclips), dim3(64), 0, s, eframe, frame_off_dev, rec);
}

}  // namespace nhans
