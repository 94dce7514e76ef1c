// Drift-aware alignment on the device: the delay of an estimate e (ne samples) against a target t tracked over the clip in
// blocks, and the warp that takes a fitted line out of the estimate (include/nhans_hip.h: nhans_drift_track,
// nhans_drift_warp, where the definition is stated in full).  All signals are float32; every
// operation is in double, one IEEE operation rounded to nearest each: the file is compiled with contraction off, and a
// fused multiply-add is written __fma_rn.
//
//   1. drift_track   one workgroup per segment: the lag vector of a block of 4,096 target samples around its centre lag,
//                    the integer peak, the fine peak on a grid of 1/32 sample with a parabola through it, the block's
//                    energy centroid and the confidence; one record of kDriftFields doubles.
//   2. drift_warp    y[u] = the estimate at p(u) = a + u + b u, by a Kaiser-windowed sinc of 32 taps whose coefficients are
//                    interpolated linearly between the 512 rows of the table; one launch for every clip of a call.
//
// The order of every sum is fixed relative to the block's first sample, so a record is a function of the pair, of the
// segment and of the centre lag alone -- and c[d] of the pair, the segment and d alone --, not of R, of the place in the
// batch, of neighbours, of the alignment of the first samples or of the run:
//   * c[d] = sum_i e[u0 + i + d] t[u0 + i] over the block's i = 0 ... 4095, a sample of e outside [0, ne) being a zero that is
//     never fetched: two tiles of kDriftTile = 2,048 samples anchored at the block's first sample; a tile's part is one
//     __fma_rn chain from +0.0 over its i ascending; c[d] = (part of tile 0) + (part of tile 1), one addition.  The
//     products of two float32 values are exact in double;
//   * E_t = sum t^2, N = sum i t^2 and E_e = sum e[u0 + i + d*]^2 over the block: thread l of 256 takes i = l, l + 256, ... in
//     one chain from +0.0 (sq = v v, exact; E: acc = acc + sq; N: acc = fma(i, sq, acc)), then the tree 128, ..., 1 through LDS;
//   * a fine value is one __fma_rn chain from +0.0 over the taps k = -15 ... 16 ascending, acc = fma(c[m + k], G[row][k], acc); a
//     lag outside the vector (only m + 16 of the last fine position can be: its weight is exactly 0) is passed over;
//   * the peaks are found with a comparison that is a total order on (value, index), so the shape of its reduction does
//     not show.
// No floating-point atomics.  Samples are fetched with single 4-byte loads, and only samples inside a clip are ever fetched.
//
// The table in the warp: read through the cache, not staged in LDS.  G and D are 262 KB together -- more than a CU's LDS
// --, and the rows a workgroup needs are a range that depends on a and b: the phase moves by b Q rows per output, so the
// 64 lanes of a wavefront read, at one column, about 4 neighbouring rows at 100 ppm and up to 33 at |b| = 2^-10, and a
// workgroup's 1,024 outputs from a handful of rows up to all 513 (wrapping from row 511 to row 0 wherever p passes an
// integer).  A staged form -- those rows of G in LDS, D formed from them -- was not built, so the two were NOT measured
// against each other; profiles/drift/README.md has the time of this one.
#include "score_common.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace nhans {

namespace {

constexpr int kDriftNT = 2 * kDriftT;                                       // taps of a row
constexpr int kDriftMaxLags = 2 * (kDriftMaxR + kDriftT) + 1;               // 2,081
constexpr int kDriftWin = kDriftBlock + kDriftMaxLags - 1;                  // samples of e a block meets over its lags
constexpr int kDriftNFine = 2 * kDriftFine + 1;
static_assert(kDriftBlock == 2 * kDriftTile && kDriftBlock % 256 == 0 && kDriftNFine <= 256, "drift_track's blocking");

// power series sum_k ((x/2)^k / k!)^2 (the series of resample.hip's bessel_i0): every term positive
double drift_bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// (v, d) before (bv, bd): the larger value; of equal values the smaller |d|; of -d and +d the non-negative one (the order
// of align.hip's align_before)
__device__ __forceinline__ bool drift_before(double v, int d, double bv, int bd) {
    if (v != bv) return v > bv;
    const int a = d < 0 ? -d : d, b = bd < 0 ? -bd : bd;
    return a != b ? a < b : d > bd;
}

// the sum of every thread's v by the tree 128, ..., 1 (every thread calls; every thread gets the sum)
__device__ __forceinline__ double drift_tree(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] = __dadd_rn(red[tid], red[tid + off]);
        __syncthreads();
    }
    return red[0];
}

// One workgroup per segment.  Staged as float32 (the conversion to double is exact wherever it happens): the block of t and
// samples [u0 + z - R - T, ... + 4096 + nl - 1) of e, zeros outside [0, ne).  A thread owns lags tid, tid + 256, ... and runs
// the two tiles' chains of a lag side by side.  LDS: 16 + 24.1 + 16.3 + 3.6 KB = 60 KB, two workgroups per CU.
__global__ void __launch_bounds__(256) drift_track_kernel(const DriftSeg* __restrict__ segs, int R, const double* __restrict__ tab,
                                                          double* __restrict__ rec, double* __restrict__ corr) {
    __shared__ float ts[kDriftBlock];
    __shared__ float es[kDriftWin];
    __shared__ double cs[kDriftMaxLags];
    __shared__ double red[256];
    __shared__ int redd[256];
    __shared__ double fine[kDriftNFine];
    const int tid = threadIdx.x;
    const DriftSeg sg = segs[blockIdx.x];
    const int nl = 2 * (R + kDriftT) + 1;
    const long long x0 = sg.u0 + (long long)sg.z - R - kDriftT;             // the sample of e at es[0]
    for (int i = tid; i < kDriftBlock; i += 256) ts[i] = sg.tgt[i];
    for (int i = tid; i < kDriftBlock + nl - 1; i += 256) {
        const long long x = x0 + i;
        es[i] = x >= 0 && x < sg.ne ? sg.est[x] : 0.f;
    }
    __syncthreads();
    for (int l = tid; l < nl; l += 256) {
        const float* __restrict__ ep = es + l;
        double p0 = 0.0, p1 = 0.0;
#pragma unroll 8
        for (int i = 0; i < kDriftTile; ++i) {
            p0 = __fma_rn((double)ep[i], (double)ts[i], p0);
            p1 = __fma_rn((double)ep[i + kDriftTile], (double)ts[i + kDriftTile], p1);
        }
        cs[l] = __dadd_rn(p0, p1);
    }
    // the block's energy and first moment
    double aE = 0.0, aN = 0.0;
    for (int i = tid; i < kDriftBlock; i += 256) {
        const double v = (double)ts[i], sq = __dmul_rn(v, v);
        aE = __dadd_rn(aE, sq);
        aN = __fma_rn((double)i, sq, aN);
    }
    const double Et = drift_tree(aE, red);           // (its first barrier also ends the writes of cs)
    const double Nt = drift_tree(aN, red);
    if (corr) {
        double* __restrict__ o = corr + (size_t)blockIdx.x * nl;
        for (int l = tid; l < nl; l += 256) o[l] = cs[l];
    }
    // the integer peak over z - R ... z + R, relative to z
    double bv = -HUGE_VAL;
    int bd = 0x7fffffff;
    for (int r = tid - R; r <= R; r += 256) {
        const double v = cs[r + R + kDriftT];
        if (drift_before(v, r, bv, bd)) { bv = v; bd = r; }
    }
    __syncthreads();
    red[tid] = bv; redd[tid] = bd;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off && drift_before(red[tid + off], redd[tid + off], red[tid], redd[tid])) { red[tid] = red[tid + off]; redd[tid] = redd[tid + off]; }
        __syncthreads();
    }
    // d* - z.  No lag wins where every value is NaN (samples that are not finite: the record is unspecified, the indices
    // below are not): the centre then stands in.
    const int dr = redd[0] < -R || redd[0] > R ? 0 : redd[0];
    // the estimate's energy over the samples paired at d*
    double aQ = 0.0;
    for (int i = tid; i < kDriftBlock; i += 256) {
        const double v = (double)es[i + dr + R + kDriftT];
        aQ = __dadd_rn(aQ, __dmul_rn(v, v));
    }
    const double Ee = drift_tree(aQ, red);
    // the fine values at d* + k / 32, k = tid - 32
    if (tid < kDriftNFine) {
        const int k = tid - kDriftFine;
        const int whole = k >= 0 ? k / kDriftFine : -((-k + kDriftFine - 1) / kDriftFine);      // floor(k / 32)
        const int row = (kDriftQ / kDriftFine) * (k - kDriftFine * whole);
        const int lm = dr + R + kDriftT + whole;                            // where lag m = d* + whole is in cs
        const double* __restrict__ g = tab + (size_t)row * kDriftNT;
        double acc = 0.0;
        for (int j = 0; j < kDriftNT; ++j) {
            const int l = lm + j - (kDriftT - 1);
            if (l >= 0 && l < nl) acc = __fma_rn(cs[l], g[j], acc);
        }
        fine[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double fv = -HUGE_VAL;
        int fk = 0x7fffffff;
        for (int i = 0; i < kDriftNFine; ++i)
            if (drift_before(fine[i], i - kDriftFine, fv, fk)) { fv = fine[i]; fk = i - kDriftFine; }
        if (fk > kDriftFine) { fk = 0; fv = fine[kDriftFine]; }           // (every fine value NaN: as above)
        double delta = 0.0;
        if (fk > -kDriftFine && fk < kDriftFine) {
            const double vm = fine[fk + kDriftFine - 1], vp = fine[fk + kDriftFine + 1];
            const double den = __dadd_rn(__dsub_rn(vm, 2.0 * fv), vp);
            if (den < 0.0) {
                delta = __ddiv_rn(__dsub_rn(vm, vp), 2.0 * den) * (1.0 / kDriftFine);
                const double lim = 0.5 / kDriftFine;
                delta = delta > lim ? lim : delta < -lim ? -lim : delta;
            }
        }
        const long long dstar = (long long)sg.z + dr;
        int flags = 0;
        if (dr == R || dr == -R || fk == kDriftFine || fk == -kDriftFine) flags |= 1;
        if (Et == 0.0 || Ee == 0.0) flags |= 2;
        double* __restrict__ o = rec + (size_t)blockIdx.x * kDriftFields;
        o[0] = __dadd_rn((double)sg.u0, __ddiv_rn(Nt, Et));
        o[1] = __dadd_rn((double)dstar + (double)fk * (1.0 / kDriftFine), delta);
        o[2] = __ddiv_rn(fv, sqrt(__dmul_rn(Ee, Et)));
        o[3] = Et; o[4] = fv; o[5] = (double)dstar; o[6] = (double)flags; o[7] = (double)sg.z;
    }
}

// One workgroup: kDriftWarpTile outputs of one clip, four per thread, neighbouring threads on neighbouring outputs.
__global__ void __launch_bounds__(256) drift_warp_kernel(const DriftWarp* __restrict__ jobs, int njobs, const double* __restrict__ tab) {
    const long long blk = blockIdx.x;
    const DriftWarp job = jobs[find_run<DriftWarp, &DriftWarp::tile0>(jobs, njobs, blk)];
    const long long i0 = (blk - job.tile0) * kDriftWarpTile;
    const int n = (int)(job.n - i0 < kDriftWarpTile ? job.n - i0 : kDriftWarpTile);
    const double* __restrict__ G = tab;
    const double* __restrict__ D = tab + kDriftTableG;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double u = (double)(job.u_lo + i0 + i);
        const double p = drift_pos(job.a, job.b, u);
        const double fl = floor(p);
        const long long m = (long long)fl;
        const double fq = __dmul_rn(__dsub_rn(p, fl), (double)kDriftQ);      // (exact: p - floor(p) is, and Q is a power of two)
        int q = (int)fq;
        if (q > kDriftQ - 1) q = kDriftQ - 1;
        const double lam = __dsub_rn(fq, (double)q);
        const double* __restrict__ g = G + (size_t)q * kDriftNT;
        const double* __restrict__ d = D + (size_t)q * kDriftNT;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < kDriftNT; ++j) {
            const long long x = m + j - (kDriftT - 1);
            const double ev = x >= 0 && x < job.ne ? (double)job.est[x] : 0.0;
            acc = __fma_rn(ev, __fma_rn(lam, d[j], g[j]), acc);
        }
        job.dst[i0 + i] = (float)acc;
    }
}

}  // namespace

// G[q][k] = sinc(x) kaiser(x / T; beta = 10), x = k - q / Q; row 0 the exact unit impulse; D[q][k] = G[q + 1][k] - G[q][k]
void drift_table(double* g, double* d) {
    const double pi = 3.14159265358979323846, beta = 10.0;
    const double i0b = drift_bessel_i0(beta);
    std::vector<double> G((size_t)kDriftTableG);
    for (int q = 0; q <= kDriftQ; ++q)
        for (int j = 0; j < kDriftNT; ++j) {
            const int k = j - (kDriftT - 1);
            double v;
            if (q == 0) v = k == 0 ? 1.0 : 0.0;
            else {
                const double x = (double)k - (double)q / (double)kDriftQ, r = x / (double)kDriftT;
                const double a = pi * x;
                const double sinc = x == 0.0 ? 1.0 : std::sin(a) / a;
                v = sinc * (drift_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b);
            }
            G[(size_t)q * kDriftNT + j] = v;
        }
    if (g) std::copy(G.begin(), G.end(), g);
    if (d)
        for (size_t i = 0; i < (size_t)kDriftTableD; ++i) d[i] = G[i + kDriftNT] - G[i];
}

void launch_drift_track(const char* kernel, const DriftSeg* segs_dev, int nsegs, int R, const double* tab, double* rec, double* corr,
                        hipStream_t s) {
    if (nsegs <= 0) return;
    if (R < 1 || R > kDriftMaxR) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, drift_track_kernel, dim3((unsigned)nsegs), dim3(256), 0, s, segs_dev, R, tab, rec, corr);
}

void launch_drift_warp(const char* kernel, const DriftWarp* jobs_dev, int njobs, long long ntiles, const double* tab, hipStream_t s) {
    if (!tiles_ok(kernel, njobs, ntiles)) return;
    NHANS_LAUNCH(kernel, drift_warp_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, jobs_dev, njobs, tab);
}

}  // namespace nhans
