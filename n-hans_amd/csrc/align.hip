// Delay estimation on the device: the cross-correlation of an estimate e (ne samples) and a target t (nt samples) over the
// lags -D ... D, the lag of its largest value and the ragged copy that cuts a pair to its common part (include/nhans_hip.h:
// nhans_align, nhans_align_cut, where the definition is stated in full).  All signals are float32;
// every operation is in double.
//
//   1. align_corr   per clip and lag d: c[d] = sum_u e[u + d] t[u] over u in [max(0, -d), min(nt, ne - d)).
//   2. align_pick   per clip: See = sum e^2, Stt = sum t^2, the lag of the largest c[d] by the tie rule, the record.
//   3. align_cut    the ragged copy of nhans_align_cut: one launch for every piece of a call.
//
// The order of every sum is fixed relative to the pair's first samples, so c[d] is a function of the pair and of d alone --
// not of D, of the pair's place in the batch, its neighbours, the alignment of its first samples or the run:
//   * the target's samples are walked in tiles of kAlignTile = 2,048, tile k being u in [2048 k, 2048 k + 2048): the tiles
//     are anchored at u = 0 whatever d is;
//   * a tile's part of c[d] is one __fma_rn chain from +0.0 over the tile's u ascending (a sample outside either clip is a
//     zero, which leaves the chain's value as it is); c[d] adds the tiles' parts one after the other, ascending, from +0.0
//     (a tile that meets no sample of e at any lag of the workgroup is passed over: its part is +0.0, which changes nothing);
//   * See and Stt: thread l of 256 adds the squares of samples l, l + 256, ... in one __fma_rn chain from +0.0, then the
//     tree 128, ..., 1 through LDS;
//   * the largest value is found with a comparison that is a total order on (value, lag), so the shape of its reduction
//     does not show.
// No floating-point atomics, and no reduction whose shape depends on the batch or on D.  Samples are fetched with single
// 4-byte loads, and only samples inside a clip are ever fetched.
#include "score_common.h"

#include <cmath>

namespace nhans {

namespace {

// A thread owns kAlignRL consecutive lags and takes kAlignRU consecutive u per step.
constexpr int kAlignRL = 8, kAlignRU = 8;
static_assert(kAlignLagBlock == 256 * kAlignRL && kAlignTile % kAlignRU == 0 && kAlignRL == 8 && kAlignRU == 8, "align_corr's blocking");
constexpr int kAlignWin = kAlignTile + kAlignLagBlock - 1;          // samples of e one tile meets over the block's lags
// The window is stored with one spare double after every eight: sample i at i + (i >> 3).  Thread l reads samples
// 8 (step + l) + k, k < 15, which are then 9 (step + l) + k + (k >> 3): for one k the 32 lanes of a half wavefront are 9
// doubles apart -- 32 different pairs of banks -- where the plain layout would put them 8 apart, on four.
constexpr int kAlignWinPadded = kAlignWin + (kAlignWin >> 3) + 1;

// One workgroup: lags [d0, d0 + kAlignLagBlock) of one clip, d0 = -D + kAlignLagBlock * block, over all of the clip's tiles;
// the running sums stay in registers from the first tile to the last.  Staged as doubles, converted once: the tile of t
// (zeros past nt) and samples [2048 k + d0, 2048 k + d0 + kAlignWin) of e (zeros outside [0, ne)).  Per step a thread
// reads eight new doubles of e -- seven of the fifteen it needs it still holds from the step before -- and the eight of t,
// one address for the whole wavefront: sixteen LDS reads for sixty-four products.  LDS: 2,048 + 4,607 doubles = 53,240
// bytes, three workgroups per CU.
__global__ void __launch_bounds__(256) align_corr_kernel(const AlignRun* __restrict__ runs, int nblk, int D, double* __restrict__ corr) {
    __shared__ double ts[kAlignTile];
    __shared__ double es[kAlignWinPadded];
    const int tid = threadIdx.x;
    const int clip = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const AlignRun run = runs[clip];
    const int nlags = 2 * D + 1;
    const long long d0 = (long long)blk * kAlignLagBlock - D;
    const int lag0 = blk * kAlignLagBlock + kAlignRL * tid;             // index of this thread's first lag in the clip's vector
    const bool active = lag0 < nlags;
    const long long dlast = d0 + kAlignLagBlock - 1 < D ? d0 + kAlignLagBlock - 1 : D;    // the block's last lag
    double sum[kAlignRL];
#pragma unroll
    for (int j = 0; j < kAlignRL; ++j) sum[j] = 0.0;
    const long long ntiles = (run.nt + kAlignTile - 1) / kAlignTile;
    for (long long k = 0; k < ntiles; ++k) {
        const long long u0 = k * kAlignTile;
        const int nu = (int)(run.nt - u0 < kAlignTile ? run.nt - u0 : kAlignTile);
        // the samples of e this tile meets over the block's lags: [u0 + d0, u0 + nu - 1 + dlast]
        if (u0 + d0 >= run.ne || u0 + nu - 1 + dlast < 0) continue;     // (the whole workgroup)
        __syncthreads();
        for (int i = tid; i < kAlignTile; i += 256) ts[i] = i < nu ? (double)run.tgt[u0 + i] : 0.0;
        for (int i = tid; i < kAlignWin; i += 256) {
            const long long x = u0 + d0 + i;
            es[i + (i >> 3)] = x >= 0 && x < run.ne ? (double)run.est[x] : 0.0;
        }
        __syncthreads();
        if (!active) continue;
        const int steps = (nu + kAlignRU - 1) / kAlignRU;
        const double* __restrict__ ep = es + 9 * tid;
        double acc[kAlignRL], w[kAlignRL + kAlignRU - 1];
#pragma unroll
        for (int j = 0; j < kAlignRL; ++j) acc[j] = 0.0;
#pragma unroll
        for (int q = 0; q < kAlignRL - 1; ++q) w[q] = ep[q];
#pragma unroll 2
        for (int it = 0; it < steps; ++it) {
            const double* __restrict__ p = ep + 9 * it;
            const double* __restrict__ tp = ts + kAlignRU * it;
            double tv[kAlignRU];
#pragma unroll
            for (int q = kAlignRL - 1; q < kAlignRL + kAlignRU - 1; ++q) w[q] = p[q + (q >> 3)];
#pragma unroll
            for (int r = 0; r < kAlignRU; ++r) tv[r] = tp[r];
#pragma unroll
            for (int r = 0; r < kAlignRU; ++r) {
#pragma unroll
                for (int j = 0; j < kAlignRL; ++j) acc[j] = __fma_rn(w[j + r], tv[r], acc[j]);
            }
#pragma unroll
            for (int q = 0; q < kAlignRL - 1; ++q) w[q] = w[q + kAlignRU];
        }
#pragma unroll
        for (int j = 0; j < kAlignRL; ++j) sum[j] = __dadd_rn(sum[j], acc[j]);
    }
    if (!active) return;
    double* __restrict__ o = corr + (size_t)clip * nlags + lag0;
#pragma unroll
    for (int j = 0; j < kAlignRL; ++j)
        if (lag0 + j < nlags) o[j] = sum[j];
}

// red[0] = sum x^2 in the order the head of the file states (every thread calls)
__device__ __forceinline__ double align_energy(const float* __restrict__ x, long long n, double* red) {
    const int tid = threadIdx.x;
    double a = 0.0;
    for (long long i = tid; i < n; i += 256) {
        const double v = (double)x[i];
        a = __fma_rn(v, v, a);
    }
    __syncthreads();
    red[tid] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] = __dadd_rn(red[tid], red[tid + off]);
        __syncthreads();
    }
    return red[0];
}

// (v, d) before (bv, bd): the larger value; of equal values the smaller |d|; of -d and +d the non-negative one
__device__ __forceinline__ bool align_before(double v, int d, double bv, int bd) {
    if (v != bv) return v > bv;
    const int a = d < 0 ? -d : d, b = bd < 0 ? -bd : bd;
    return a != b ? a < b : d > bd;
}

// One workgroup per clip.  A thread without a lag holds (-inf, INT_MAX), which every lag comes before.
__global__ void __launch_bounds__(256) align_pick_kernel(const AlignRun* __restrict__ runs, int D, const double* __restrict__ corr,
                                                         double* __restrict__ rec) {
    __shared__ double red[256];
    __shared__ int redd[256];
    const int tid = threadIdx.x, nlags = 2 * D + 1;
    const AlignRun run = runs[blockIdx.x];
    const double See = align_energy(run.est, run.ne, red);
    const double Stt = align_energy(run.tgt, run.nt, red);
    const double* __restrict__ c = corr + (size_t)blockIdx.x * nlags;
    double bv = -HUGE_VAL;
    int bd = 0x7fffffff;
    for (int i = tid; i < nlags; i += 256) {
        const double v = c[i];
        if (align_before(v, i - D, bv, bd)) { bv = v; bd = i - D; }
    }
    __syncthreads();
    red[tid] = bv; redd[tid] = bd;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off && align_before(red[tid + off], redd[tid + off], red[tid], redd[tid])) { red[tid] = red[tid + off]; redd[tid] = redd[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double peak = red[0];
        const long long d = redd[0];
        long long nc = run.ne - (d > 0 ? d : 0) < run.nt - (d < 0 ? -d : 0) ? run.ne - (d > 0 ? d : 0) : run.nt - (d < 0 ? -d : 0);
        if (nc < 0) nc = 0;
        double* __restrict__ o = rec + (size_t)blockIdx.x * kAlignFields;
        o[0] = (double)run.ne; o[1] = (double)run.nt; o[2] = (double)D; o[3] = (double)d; o[4] = peak;
        o[5] = peak / sqrt(__dmul_rn(See, Stt)); o[6] = (double)nc; o[7] = 0.0;
    }
}

// One workgroup: kAlignCutTile samples of one piece.
__global__ void __launch_bounds__(256) align_cut_kernel(const AlignCopy* __restrict__ jobs, int njobs) {
    const long long b = blockIdx.x;
    const AlignCopy job = jobs[find_run<AlignCopy, &AlignCopy::tile0>(jobs, njobs, b)];
    const long long i0 = (b - job.tile0) * kAlignCutTile;
    const int n = (int)(job.n - i0 < kAlignCutTile ? job.n - i0 : kAlignCutTile);
    for (int i = threadIdx.x; i < n; i += 256) job.dst[i0 + i] = job.src[i0 + i];
}

}  // namespace

void launch_align_corr(const char* kernel, const AlignRun* runs_dev, int nruns, int D, double* corr, hipStream_t s) {
    if (nruns <= 0) return;
    if (D < 0 || D > kAlignMaxLag) { note_refusal(kernel); return; }
    const int nblk = (2 * D + 1 + kAlignLagBlock - 1) / kAlignLagBlock;
    if ((long long)nruns * nblk > 0x7fffffffLL) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, align_corr_kernel, dim3((unsigned)(nruns * nblk)), dim3(256), 0, s, runs_dev, nblk, D, corr);
}

void launch_align_pick(const char* kernel, const AlignRun* runs_dev, int nruns, int D, const double* corr, double* rec, hipStream_t s) {
    if (nruns <= 0) return;
    if (D < 0 || D > kAlignMaxLag) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, align_pick_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, D, corr, rec);
}

void launch_align_cut(const char* kernel, const AlignCopy* jobs_dev, int njobs, long long ntiles, hipStream_t s) {
    if (!tiles_ok(kernel, njobs, ntiles)) return;
    NHANS_LAUNCH(kernel, align_cut_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, jobs_dev, njobs);
}

}  // namespace nhans
