// Phase refinement (include/nhans_hip.h: nhans_phase_*): one Griffin-Lim projection d = P(A, t) per launch, without the
// waveform ever reaching HBM.
//
//   phase_project_kernel : c = A u(t) -> inverse transform, synthesis window, overlap-add (istft_ola_kernel's arithmetic)
//                          -> analysis window, forward real-input transform (stft_features_kernel's arithmetic) -> d, the
//                          momentum step t' = d + alpha (d - d_prev), and a frame's sum (|d| - A)^2
//   phase_prepare_kernel : A = exp(logmag) once per call, t_0 = cos ph + i sin ph, a frame's sum A^2
//   phase_angle_kernel   : angle(t) of the last state
//   phase_inc_kernel     : a clip's inconsistency from the frame partials
//
// The projection follows the design of stft.hip.  Persistent workgroups walk runs of kPhaseRun = 20 frames of a clip.  A
// run's samples are the hops f0 ... f0 + 21 (the last one to its 80th sample), which frames f0 - 2 ... f0 + 21 overlap: 24
// frames = 4 waves x 3 complex transforms x 2 frames, one pass of the inverse kernel's shape.  Their windowed frames land
// in the LDS buffer that aliases the (wavefront-private) transform areas; the run's 3,440 samples are overlap-added from it
// in gather form into a span of their own; then the areas become the forward transform's transpose buffer: 400 pass-1
// tasks (frame x column) and 220 pass-2 tasks (frame x row) on the 256 lanes, the bins written from the pass-2 registers.
// Halo frames are transformed again by the neighbouring run (24 inverse transforms per 20 frames): the price of keeping
// 2 x 1,608 bytes per frame of waveform traffic and a launch boundary out of every iteration.
// Inside an iteration there is no log, atan2, sine or cosine: u(t) is one reciprocal square root.  Measured on 256 x 998
// frames (profiles/phase/README.md): 0.39 ms per projection, the time of one istft_ola + stft_features launch pair.
#include "stft_common.h"
#include "score_common.h"

namespace nhans {

constexpr int kPhaseFrames = kPhaseRun + 4;                         // frames f0 - 2 ... f0 + kPhaseRun + 1
constexpr int kPhaseSpan = kWin + kHop * (kPhaseRun - 1);           // 3,440 samples
constexpr int kPhaseXs = kPhaseRun * kBins > kPhaseSpan ? kPhaseRun * kBins : kPhaseSpan;   // the span, later |d| - A of the run
static_assert(kPhaseFrames == 4 * kFpw * 2, "24 frames = 4 waves x 3 transforms x 2 frames");
static_assert(kPhaseRun * 20 <= 2 * 256 && kPhaseRun * kRows <= 256, "pass 1 in two sweeps, pass 2 in one");

// z / |z|; 1 + 0j where |z| is zero or below the smallest normal number.  The components are brought into a range where
// their squares neither vanish nor overflow (a power of two: exact), then one hardware reciprocal square root, refined
// once (v_rsq_f32 is good to 1 ulp; the step leaves the rounding of the last operations only).
__device__ __forceinline__ cplx unit(cplx z) {
    const float mx = fmaxf(fabsf(z.x), fabsf(z.y));
    const float sc = mx < 9.094947017729282e-13f /* 2^-40 */ ? 18446744073709551616.f /* 2^64 */
                   : mx > 1099511627776.f /* 2^40 */ ? 3.3881317890172014e-21f /* 2^-68 */ : 1.f;
    const float x = z.x * sc, y = z.y * sc;
    const float m = fmaf(x, x, y * y);
    // |z| < 2^-126  <=>  |z| 2^64 < 2^-62  <=>  m < 2^-124
    const bool tiny = mx < 9.094947017729282e-13f && m < 4.70197740328915e-38f /* 2^-124 */;
    float r = __builtin_amdgcn_rsqf(m);
    r = r * fmaf(-0.5f * m, r * r, 1.5f);
    return tiny ? cmake(1.f, 0.f) : cmake(x * r, y * r);
}

__global__ void __launch_bounds__(256, 2) phase_project_kernel(
    const float* __restrict__ Ag, const cplx* __restrict__ tin, const int64_t* __restrict__ frame_off,
    const int* __restrict__ block_clip, const int* __restrict__ block_f0, int nblocks, const cplx* __restrict__ tw400g,
    const float* __restrict__ windowg, const float* __restrict__ wsyng, const cplx* dprev, float alpha, cplx* dout,
    cplx* __restrict__ tout, double* __restrict__ num) {
    constexpr int R = kPhaseRun, F = kPhaseFrames;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cplx* tw = reinterpret_cast<cplx*>(smem_raw);                 // 400
    float* wsyn = reinterpret_cast<float*>(tw + 400);             // 400
    float* win = wsyn + kWin;                                     // 400
    cplx* area = reinterpret_cast<cplx*>(win + kWin);             // per wave 3 x 420: spectra Z, then transpose rows
    float* y = reinterpret_cast<float*>(area);                    // [F][400] windowed frames, aliasing the areas
    cplx* tbuf = area;                                            // [R][11][21] forward transpose rows, aliasing them too
    float* xs = reinterpret_cast<float*>(area + 4 * kFpw * kTFrame);   // the run's samples; after pass 1: es[R][201] = |d| - A
    static_assert((size_t)F * kWin * sizeof(float) <= (size_t)4 * kFpw * kTFrame * sizeof(cplx), "y fits the areas");
    static_assert((size_t)R * kTReal <= (size_t)4 * kFpw * kTFrame, "tbuf fits the areas");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane / 20, q = lane - j * 20;
    const bool active = lane < 60;
    cplx* a_wave = area + wave * kFpw * kTFrame;
    const int lf0 = wave * kFpw * 2;                 // first local frame of this wave; clip frame = f0 - 2 + lf
    constexpr int NIN = (kFpw * kBins + 63) / 64;    // (transform, bin) items per lane

    // The state and the magnitudes of frames a and b of a run: all of a lane's 40 loads are issued before the first is used
    // (an item outside the clip loads element 0 of the clip and is masked out, so no load sits behind a branch).  Fetching
    // the NEXT run under the current one, as istft_ola_kernel does, was built and measured: its 60 registers spill (316
    // bytes of scratch per lane at two waves per SIMD) and a projection takes 0.60 ms instead of 0.39; at one workgroup
    // per CU nothing spills and it takes 0.57 ms (profiles/phase/README.md).
    cplx ta[NIN], tb[NIN];
    float ma[NIN], mb[NIN];
    unsigned va = 0, vb = 0;
    auto fetch = [&](int blk) {
        const int c = block_clip[blk];
        const int64_t fb_ = frame_off[c];
        const int Tc = (int)(frame_off[c + 1] - fb_);
        const int fr0 = block_f0[blk] - 2 + lf0;
        const float* __restrict__ Ac = Ag + fb_ * kBins;             // wave-uniform 64-bit bases + 32-bit element offsets per lane
        const cplx* __restrict__ tc = tin + fb_ * kBins;             // (a clip is far below 2^31 / 201 frames)
        va = 0; vb = 0;
#pragma unroll
        for (int u = 0; u < NIN; ++u) {
            const int idx = u * 64 + lane;
            const int tr = idx / kBins, k = idx - tr * kBins;
            const int fa = fr0 + 2 * tr;
            const bool oka = idx < kFpw * kBins && fa >= 0 && fa < Tc;
            const bool okb = idx < kFpw * kBins && fa + 1 >= 0 && fa + 1 < Tc;
            const unsigned oa = oka ? (unsigned)(fa * kBins + k) : 0u, ob = okb ? (unsigned)((fa + 1) * kBins + k) : 0u;
            ta[u] = tc[oa]; ma[u] = Ac[oa];
            tb[u] = tc[ob]; mb[u] = Ac[ob];
            va |= oka ? 1u << u : 0u;
            vb |= okb ? 1u << u : 0u;
        }
    };

    for (int i = tid; i < 400; i += 256) { tw[i] = tw400g[i]; wsyn[i] = wsyng[i]; win[i] = windowg[i]; }
    __syncthreads();

#pragma unroll 1
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int clip = block_clip[blk], f0 = block_f0[blk];
        const int64_t fr_beg = frame_off[clip];
        const int T = (int)(frame_off[clip + 1] - fr_beg);
        // Z = Ca + i Cb over all 400 bins from the 201 of c = A u(t) (frames outside [0, T) contribute zero)
        fetch(blk);
#pragma unroll
        for (int u = 0; u < NIN; ++u) {
            const int idx = u * 64 + lane;
            const int tr = idx / kBins, k = idx - tr * kBins;
            const cplx ua = unit(ta[u]), ub = unit(tb[u]);
            const float a = ((va >> u) & 1u) ? ma[u] : 0.f, b = ((vb >> u) & 1u) ? mb[u] : 0.f;
            cplx ca = cmake(a * ua.x, a * ua.y), cb = cmake(b * ub.x, b * ub.y);
            const bool edge = k == 0 || k == 200;
            if (edge) { ca.y = 0.f; cb.y = 0.f; }
            if (idx < kFpw * kBins) {
                cplx* z = a_wave + tr * 400;
                z[k] = cmake(ca.x - cb.y, ca.y + cb.x);
                if (!edge) z[400 - k] = cmake(ca.x + cb.y, cb.x - ca.y);
            }
        }
        wave_lds_sync();
        cplx col[20];
        if (active) {
            const cplx* z = a_wave + j * 400;
#pragma unroll
            for (int a = 0; a < 20; ++a) col[a] = z[20 * a + q];
        }
        wave_lds_sync();                             // every lane holds its column: the area becomes the transpose buffer
        if (active) {
            cplx yv[20];
            fft400_pass1<true>(col, q, tw, yv);
            cplx* tf = a_wave + j * kTFrame;
#pragma unroll
            for (int c1 = 0; c1 < 20; ++c1) tf[c1 * kTRow + q] = yv[c1];
        }
        wave_lds_sync();
        cplx x[20];
        if (active) {
            cplx row[20];
            const cplx* tf = a_wave + j * kTFrame + q * kTRow;
#pragma unroll
            for (int b = 0; b < 20; ++b) row[b] = tf[b];
            fft400_pass2<true>(row, x);
        }
        __syncthreads();                             // every wave is through with its area: it becomes y
        if (active) {
            float* ya = y + (lf0 + 2 * j) * kWin;
#pragma unroll
            for (int c2 = 0; c2 < 20; ++c2) {
                const int n = q + 20 * c2;
                const float w = (1.0f / 400.0f) * wsyn[n];
                ya[n] = x[c2].x * w;                 // real part: frame a
                ya[kWin + n] = x[c2].y * w;          // imaginary part: frame b
            }
        }
        __syncthreads();
        // gather-form overlap-add into the span: sample i of hop f0 + hl sums local frames hl, hl + 1, hl + 2 (ascending)
        {
            typedef float f32x4v __attribute__((ext_vector_type(4)));
            for (int i = tid * 4; i < kPhaseSpan; i += 1024) {
                const int hl = i / kHop, r = i - hl * kHop;
                f32x4v acc = {0.f, 0.f, 0.f, 0.f};
                if (r < kWin - 2 * kHop) acc = *reinterpret_cast<const f32x4v*>(y + hl * kWin + 2 * kHop + r);
                acc += *reinterpret_cast<const f32x4v*>(y + (hl + 1) * kWin + kHop + r);
                acc += *reinterpret_cast<const f32x4v*>(y + (hl + 2) * kWin + r);
                *reinterpret_cast<f32x4v*>(xs + i) = acc;
            }
        }
        __syncthreads();                             // y has been read: the areas become tbuf
        // pass 1: task (frame f, column n2) = real 20-point DFT over n1 of the windowed samples x[20*n1 + n2]
#pragma unroll 1
        for (int id = tid; id < R * 20; id += 256) {
            const int f = id / 20, n2 = id - f * 20;
            float colr[20];
            cplx yv[kRows];
            const float* xf = xs + f * kHop + n2;
#pragma unroll
            for (int n1 = 0; n1 < 20; ++n1) colr[n1] = xf[20 * n1] * win[20 * n1 + n2];
            fft400_pass1_real(colr, n2, tw, yv);
            cplx* tf = tbuf + f * kTReal + n2;
#pragma unroll
            for (int k1 = 0; k1 < kRows; ++k1) tf[k1 * kTRow] = yv[k1];
        }
        __syncthreads();                             // (also: the span has been read, xs becomes es)
        // pass 2: task (frame f, row k1 <= 10) = complex 20-point DFT over n2 -> X[k1 + 20*k2], k2 = 0..19
        if (tid < R * kRows) {
            const int f = tid / kRows, k1 = tid - f * kRows;
            cplx row[20], X[20];
            const cplx* tf = tbuf + f * kTReal + k1 * kTRow;
#pragma unroll
            for (int n2 = 0; n2 < 20; ++n2) row[n2] = tf[n2];
            fft400_pass2<false>(row, X);
            if (f0 + f < T) {
                const int64_t e0 = (fr_beg + f0 + f) * kBins;
                float* es = xs + f * kBins;
#pragma unroll
                for (int k2 = 0; k2 < 20; ++k2) {
                    const bool mirror = k2 >= 10 && k1 != 0;
                    const bool live = k2 < 10 || (k1 == 0 ? k2 == 10 : k1 != 10);
                    if (!live) continue;
                    const int bin = mirror ? 400 - k1 - 20 * k2 : k1 + 20 * k2;
                    const cplx d = cmake(X[k2].x, mirror ? -X[k2].y : X[k2].y);
                    if (num) es[bin] = __builtin_amdgcn_sqrtf(d.x * d.x + d.y * d.y) - Ag[e0 + bin];
                    cplx tn = d;
                    if (dprev) {
                        const cplx p = dprev[e0 + bin];
                        tn = cmake(fmaf(alpha, d.x - p.x, d.x), fmaf(alpha, d.y - p.y, d.y));
                    }
                    if (dout) dout[e0 + bin] = d;
                    if (tout) tout[e0 + bin] = tn;
                }
            }
        }
        __syncthreads();                             // tbuf has been read: the areas may be rewritten; es is complete
        if (num && tid < R && f0 + tid < T) {        // (the next run writes xs two barriers from here)
            const float* es = xs + tid * kBins;
            double acc = 0.0;
            for (int k = 0; k < kBins; ++k) { const double e = (double)es[k]; acc = fma(e, e, acc); }
            num[fr_beg + f0 + tid] = acc;
        }
    }
}

void launch_phase_project(const float* A, const float* t_in, const int64_t* frame_off_dev, const int* block_clip, const int* block_f0,
                          int nblocks, const float* tw400, const float* window, const float* wsyn, const float* d_prev, float alpha,
                          float* d_out, float* t_out, double* num, hipStream_t s) {
    if (nblocks <= 0) return;
    constexpr size_t lds = (400 + 4 * kFpw * kTFrame) * sizeof(cplx) + (2 * kWin + kPhaseXs) * sizeof(float);     // 62.8 KB
    static unsigned long long attr_devices = 0;
    set_max_dynamic_lds(reinterpret_cast<const void*>(&phase_project_kernel), lds, &attr_devices, "phase_project");
    const int grid = nblocks < 256 * 2 ? nblocks : 256 * 2;     // two resident workgroups per CU
    NHANS_LAUNCH("phase_project", phase_project_kernel, dim3(grid), dim3(256), lds, s, A, reinterpret_cast<const cplx*>(t_in),
                 frame_off_dev, block_clip, block_f0, nblocks, reinterpret_cast<const cplx*>(tw400), window, wsyn,
                 reinterpret_cast<const cplx*>(d_prev), alpha, reinterpret_cast<cplx*>(d_out), reinterpret_cast<cplx*>(t_out), num);
}

// ---------------------------------------------------------------------------------------------
// One workgroup: kPhasePrepFrames frames.  Elementwise A (and t_0), then one lane per frame sums its A^2, bins ascending.
constexpr int kPhasePrepFrames = 16;
__global__ void __launch_bounds__(256) phase_prepare_kernel(const float* __restrict__ logmag, const float* __restrict__ phase,
                                                            long long nframes, float* __restrict__ A, cplx* __restrict__ t0,
                                                            double* __restrict__ den) {
    __shared__ float as[kPhasePrepFrames * kBins];
    const long long fb = (long long)blockIdx.x * kPhasePrepFrames;
    const int nf = (int)(nframes - fb < kPhasePrepFrames ? nframes - fb : kPhasePrepFrames);
    const long long e0 = fb * kBins;
    for (int i = threadIdx.x; i < nf * kBins; i += 256) {
        const float a = fast_exp(logmag[e0 + i]);
        A[e0 + i] = a;
        as[i] = a;
        if (phase) {
            float sn, cs;
            fast_sincos(phase[e0 + i], &sn, &cs);
            t0[e0 + i] = cmake(cs, sn);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nf) {
        const float* a = as + threadIdx.x * kBins;
        double acc = 0.0;
        for (int k = 0; k < kBins; ++k) { const double v = (double)a[k]; acc = fma(v, v, acc); }
        den[fb + threadIdx.x] = acc;
    }
}

void launch_phase_prepare(const float* logmag, const float* phase, int64_t nframes, float* A, float* t0, double* den, hipStream_t s) {
    const long long nb = (nframes + kPhasePrepFrames - 1) / kPhasePrepFrames;
    if (!tiles_ok("phase_prepare", 1, nb)) return;
    NHANS_LAUNCH("phase_prepare", phase_prepare_kernel, dim3((unsigned)nb), dim3(256), 0, s, logmag, phase, (long long)nframes, A,
                 reinterpret_cast<cplx*>(t0), den);
}

__global__ void __launch_bounds__(256) phase_angle_kernel(const cplx* __restrict__ t, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const cplx v = t[i]; out[i] = fast_atan2(v.y, v.x); }
}

void launch_phase_angle(const float* t, int64_t n, float* phase_out, hipStream_t s) {
    const long long nb = (n + 255) / 256;
    if (!tiles_ok("phase_angle", 1, nb)) return;
    NHANS_LAUNCH("phase_angle", phase_angle_kernel, dim3((unsigned)nb), dim3(256), 0, s, reinterpret_cast<const cplx*>(t), (long long)n,
                 phase_out);
}

// One wavefront per clip.
__global__ void __launch_bounds__(64) phase_inc_kernel(const double* __restrict__ num, const double* __restrict__ den,
                                                       const int64_t* __restrict__ frame_off, double* __restrict__ inc_out, int stride,
                                                       int col) {
    const int clip = blockIdx.x;
    const int64_t b = frame_off[clip], e = frame_off[clip + 1];
    double sn = 0.0, sd = 0.0;
    for (int64_t f = b + threadIdx.x; f < e; f += 64) { sn = __dadd_rn(sn, num[f]); sd = __dadd_rn(sd, den[f]); }
    sn = wave_sum(sn);
    sd = wave_sum(sd);
    if (threadIdx.x == 0) inc_out[(size_t)clip * stride + col] = sd == 0.0 ? quiet_nan() : sn / sd;
}

void launch_phase_inc(const double* num, const double* den, const int64_t* frame_off_dev, int nclips, double* inc_out, int stride, int col,
                      hipStream_t s) {
    if (!tiles_ok("phase_inc", nclips, nclips)) return;
    NHANS_LAUNCH("phase_inc", phase_inc_kernel, dim3(nclips), dim3(64), 0, s, num, den, frame_off_dev, inc_out, stride, col);
}

}  // namespace nhans
