// Level meter and automatic compensation of a live session, and their whole-clip twin (include/nhans_hip.h:
// nhans_level_*).
//
// Per hop h of a slot's 16 kHz output -- samples [160 h, 160 h + 160) of the denoised stream d and the mixed round trip
// m, r = __fsub_rn(m, d) -- three powers in double: Pd = sum double(d)^2, Pr = sum double(r)^2, Pm = sum double(m)^2.
// A product of two float32 is exact in double (so a product fused into its sum rounds as the two operations do), and ONE
// function sums a hop (hop_powers: one wavefront, lane k adds samples k, k + 64, k + 128 in that order, then the
// __shfl_down tree 32, 16, ..., 1), so a power's bits are a property of the recording.  From the powers of a trailing
// window of W hops (W = 0: every hop since h0, a sequential running sum) the gain of hop h is the reference's automatic
// compensation, SN/apply.py write_snc_outputs:
//     g = (Sd / Sr) / 20,   w_h = float32(min(max(g, 0), wmax)),   0 where Sr == 0 or g is NaN,
// every sum formed in ascending hop order, whether a term comes from the carried state or from this push.
#include "score_common.h"

namespace nhans {

namespace {

// The powers of one hop of cnt <= 160 samples at d / m, by one whole wavefront; the result is lane 0's.
__device__ __forceinline__ void hop_powers(const float* __restrict__ d, const float* __restrict__ m, int cnt, int lane,
                                           double* pd, double* pr, double* pm) {
    double ad = 0.0, ar = 0.0, am = 0.0;
    for (int k = lane; k < cnt; k += 64) {
        const float dv = d[k], mv = m[k];
        const double dd = (double)dv, dr = (double)__fsub_rn(mv, dv), dm = (double)mv;
        ad = __dadd_rn(ad, __dmul_rn(dd, dd));
        ar = __dadd_rn(ar, __dmul_rn(dr, dr));
        am = __dadd_rn(am, __dmul_rn(dm, dm));
    }
    *pd = wave_sum(ad); *pr = wave_sum(ar); *pm = wave_sum(am);
}

// One workgroup per run, 256 hops per round.  LDS: the powers of the last 512 hops, hop j at j mod 512 -- a window
// reaches at most 255 hops back, so while a round writes its 256 entries the 256 before them are all still there.
// Phase 1: the four wavefronts take the round's hops in turn.  Phase 2: thread t takes hop hb + t, forms the running sums
// (the carry of the round before plus the round's powers up to its hop, one after the other) and the window sums, the
// gain, and -- the last hop's thread -- the meter.
__global__ void __launch_bounds__(256) level_kernel(const LevelRun* __restrict__ runs) {
    __shared__ double pw[3][2 * kLevelRing];
    __shared__ double carry[3];
    const LevelRun r = runs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long H0 = r.hop_first, H1 = H0 + r.nh;
    constexpr int kMask = 2 * kLevelRing - 1;
    {
        const long long j = H0 - kLevelRing + tid;
        if (r.in && j >= r.h0)
            for (int q = 0; q < 3; ++q) pw[q][j & kMask] = r.in[q * kLevelRing + (j & (kLevelRing - 1))];
        if (tid < 3) carry[tid] = (r.in && H0 > r.h0) ? r.in[kLevelSums + tid] : 0.0;
    }
    for (long long hb = H0; hb < H1; hb += kLevelRing) {
        const int nb = (int)(H1 - hb < kLevelRing ? H1 - hb : kLevelRing);
        for (int t = wave; t < nb; t += 4) {
            const long long h = hb + t, off = (h - H0) * kHop;
            const long long left = r.n_new - off;
            double pd, pr, pm;
            hop_powers(r.den + off, r.mix + off, (int)(left < kHop ? left : kHop), lane, &pd, &pr, &pm);
            if (lane == 0) { pw[0][h & kMask] = pd; pw[1][h & kMask] = pr; pw[2][h & kMask] = pm; }
        }
        __syncthreads();
        double run[3] = {0.0, 0.0, 0.0};
        if (tid < nb) {
            const long long h = hb + tid;
            double S[3];
            for (int q = 0; q < 3; ++q) {
                double a = carry[q];
                for (long long j = hb; j <= h; ++j) a = __dadd_rn(a, pw[q][j & kMask]);
                run[q] = a;
                if (r.W > 0) {
                    const long long lo = h - r.W + 1 > r.h0 ? h - r.W + 1 : r.h0;
                    a = 0.0;
                    for (long long j = lo; j <= h; ++j) a = __dadd_rn(a, pw[q][j & kMask]);
                }
                S[q] = a;
            }
            const double g = (S[0] / S[1]) / 20.0;
            float w = 0.f;
            if (S[1] != 0.0 && g == g) w = (float)fmin(fmax(g, 0.0), r.wmax);
            r.wtab[h - H0] = w;
            if (h == H1 - 1 && r.meter) {
                r.meter[0] = S[0]; r.meter[1] = S[1]; r.meter[2] = S[2];
                r.meter[3] = (double)(H1 - r.h0);
                r.meter[4] = (double)w;
                r.meter[5] = S[0] / S[1];
                r.meter[6] = 0.0; r.meter[7] = 0.0;
            }
        }
        __syncthreads();
        if (tid == nb - 1)
            for (int q = 0; q < 3; ++q) carry[q] = run[q];
    }
    __syncthreads();
    if (r.out) {
        const long long j = H1 - kLevelRing + tid;
        if (j >= r.h0)
            for (int q = 0; q < 3; ++q) r.out[q * kLevelRing + (j & (kLevelRing - 1))] = pw[q][j & kMask];
        if (tid < 3) r.out[kLevelSums + tid] = carry[tid];
    }
}

}  // namespace

void launch_level(const char* kernel, const LevelRun* runs_dev, int nruns, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, level_kernel, dim3(nruns), dim3(256), 0, s, runs_dev);
}

}  // namespace nhans
