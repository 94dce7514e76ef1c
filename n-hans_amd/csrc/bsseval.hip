// BSS Eval on the device: SDR, SIR and SAR of an estimate e against a target s_0 and (J = 2) an interferer s_1, each allowed
// a filter of L taps (include/nhans_hip.h: nhans_bss_eval, where the definition is stated in full).
// All signals are float32, n common samples, zero outside [0, n); every operation is in double.  M = J L.
//
//   1. bss_corr      per tile of kBssCorrTile samples t and lag 0 <= d < L, the tile's part of the six sums
//                        r00[d] = sum s_0[t] s_0[t + d]   r10[d] = sum s_1[t] s_0[t + d]   r01[d] = sum s_0[t] s_1[t + d]
//                        r11[d] = sum s_1[t] s_1[t + d]   q0[d]  = sum s_0[t] e[t + d]     q1[d]  = sum s_1[t] e[t + d]
//                    (J = 1: r00 and q0 only).  r_01 at a negative lag -d is r10[d]; r_00 and r_11 are even.
//   2. bss_reduce    per clip and sum: the tiles' parts added.
//   3. bss_gram      the lower triangle of G, column-major: G[(j,a),(k,b)] = r_jk[a - b].
//   4. bss_chol      one workgroup per clip: G = R R^T (R lower, no pivoting), R y = D, R^T C = y, and -- the leading L x L
//                    block of R being the factor of the leading block of G, its first L columns never see the others --
//                    R_00^T C0 = y[:L] for the target-only filter.  The pivot rule of the header flags a singular clip.
//   5. bss_project   per tile of kBssProjTile samples t of [0, n + L - 1): P[t], s_target[t] and the six squared terms.
//   6. bss_finish    per clip: the tiles' energies added, the figures, the record.
//
// The order of every sum is fixed relative to the clip's first sample, so a record's bits are a property of the clip tuple
// and of L -- not of its place in the batch, its group, its neighbours, the alignment of its first sample or the run:
//   * a tile's part of a sum is one __fma_rn chain from +0.0 over the tile's samples t ascending (samples past n are
//     zeros, which leave the chain's value as it is); a clip's sum adds its tiles' parts one after the other, ascending;
//   * a trailing element of the factorisation takes its kBssPanel products of one panel in one __fma_rn chain, column of
//     the panel ascending, panels ascending; inside a panel a column is updated by the columns before it, ascending; a
//     column is divided by the root of its pivot;
//   * R y = D: y[k] = v[k] / R[k][k], then v[i] = fma(-R[i][k], y[k], v[i]) for i > k, k ascending.  R^T x = y, k descending:
//     thread l of 256 adds R[i][k] x[i] for i = k + 1 + l, k + 1 + l + 256, ... in one chain, a wavefront adds its lanes by
//     the __shfl_down tree 32, ..., 1, the four wavefronts' sums are added in order, x[k] = (y[k] - sum) / R[k][k];
//   * P[t] is one __fma_rn chain over source 0's taps b ascending, then source 1's; s_target[t] one over C0's taps;
//   * a tile's energy: thread l adds the squares of t = l, l + 256, l + 512, l + 768 of the tile in that order, then the
//     tree 128, ..., 1 through LDS; a clip's energy adds its tiles' one after the other, ascending.
// No floating-point atomics, and no reduction whose shape depends on the batch.  Samples are fetched with single 4-byte
// loads, and only samples [0, n) of a clip are ever fetched.
#include "score_common.h"

#include <cmath>

namespace nhans {

namespace {

constexpr int kBssMaxM = 2 * kBssMaxL;
constexpr int kBssCorrWin = kBssCorrTile + kBssMaxL - 1, kBssProjWin = kBssProjTile + kBssMaxL - 1;

// One workgroup: one tile of one clip, all three signals staged as doubles with the L - 1 samples after the tile; thread l
// owns the lags l and l + 256.  The products' left factors s_0[t], s_1[t] are one address for the whole wavefront, the right
// factors consecutive doubles: no bank conflict.  LDS: 3 x 2,559 doubles = 61,416 bytes, two workgroups per CU.
__global__ void __launch_bounds__(256) bss_corr_kernel(const BssRun* __restrict__ runs, int nruns, int L, int J, double* __restrict__ part) {
    __shared__ double sig[3][kBssCorrWin];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const BssRun run = runs[find_run<BssRun, &BssRun::ctile0>(runs, nruns, b)];
    const long long t0 = (b - run.ctile0) * kBssCorrTile;
    const int W = kBssCorrTile + L - 1;
    for (int i = tid; i < W; i += 256) {
        const long long t = t0 + i;
        const bool ok = t < run.n;
        sig[0][i] = ok ? (double)run.s0[t] : 0.0;
        sig[1][i] = ok && J == 2 ? (double)run.s1[t] : 0.0;
        sig[2][i] = ok ? (double)run.est[t] : 0.0;
    }
    __syncthreads();
    const int nt = (int)(run.n - t0 < kBssCorrTile ? run.n - t0 : kBssCorrTile);
    const int NI = J == 2 ? 6 : 2;
    double* __restrict__ o = part + (size_t)b * NI * L;
    for (int d = tid; d < L; d += 256) {
        const double* __restrict__ b0 = sig[0] + d;
        const double* __restrict__ b1 = sig[1] + d;
        const double* __restrict__ be = sig[2] + d;
        if (J == 2) {
            double r00 = 0.0, r10 = 0.0, r01 = 0.0, r11 = 0.0, q0 = 0.0, q1 = 0.0;
#pragma unroll 4
            for (int t = 0; t < nt; ++t) {
                const double a0 = sig[0][t], a1 = sig[1][t], x0 = b0[t], x1 = b1[t], xe = be[t];
                r00 = __fma_rn(a0, x0, r00); r10 = __fma_rn(a1, x0, r10);
                r01 = __fma_rn(a0, x1, r01); r11 = __fma_rn(a1, x1, r11);
                q0 = __fma_rn(a0, xe, q0); q1 = __fma_rn(a1, xe, q1);
            }
            o[d] = r00; o[L + d] = r10; o[2 * L + d] = r01; o[3 * L + d] = r11; o[4 * L + d] = q0; o[5 * L + d] = q1;
        } else {
            double r00 = 0.0, q0 = 0.0;
#pragma unroll 4
            for (int t = 0; t < nt; ++t) {
                const double a0 = sig[0][t];
                r00 = __fma_rn(a0, b0[t], r00);
                q0 = __fma_rn(a0, be[t], q0);
            }
            o[d] = r00; o[L + d] = q0;
        }
    }
}

// grid (clips, ceil(NI L / 256)): one thread per sum of a clip
__global__ void __launch_bounds__(256) bss_reduce_kernel(const BssRun* __restrict__ runs, int NIL, const double* __restrict__ part,
                                                         double* __restrict__ lag) {
    const int idx = blockIdx.y * 256 + threadIdx.x;
    if (idx >= NIL) return;
    const BssRun run = runs[blockIdx.x];
    const double* __restrict__ p = part + (size_t)run.ctile0 * NIL + idx;
    double a = 0.0;
    for (long long k = 0; k < run.ctiles; ++k) a = __dadd_rn(a, p[(size_t)k * NIL]);
    lag[(size_t)blockIdx.x * NIL + idx] = a;
}

// grid (clips, M): column c of the lower triangle, rows c ... M - 1
__global__ void __launch_bounds__(256) bss_gram_kernel(int L, int J, const double* __restrict__ lag, double* __restrict__ G) {
    const int M = J * L, NI = J == 2 ? 6 : 2, c = blockIdx.y;
    const double* __restrict__ lg = lag + (size_t)blockIdx.x * NI * L;
    double* __restrict__ col = G + ((size_t)blockIdx.x * M + c) * M;
    const int k = c >= L ? 1 : 0, bb = c - k * L;
    for (int i = c + threadIdx.x; i < M; i += 256) {
        const int j = i >= L ? 1 : 0, d = (i - j * L) - bb;
        double v;
        if (j == k) v = lg[(j ? 3 * L : 0) + d];            // (same block, i >= c: d >= 0)
        else v = d >= 0 ? lg[L + d] : lg[2 * L - d];        // r_10[d]: r10[d], or r01[-d]
        col[i] = v;
    }
}

// this thread's part of column k of the factor below the diagonal -- rows k + 1 + l + 256 j < m, j < 4 -- and the diagonal
__device__ __forceinline__ void bss_column(const double* __restrict__ A, int M, int m, int k, double (&c)[4], double& d) {
    const double* __restrict__ col = A + (size_t)k * M;
    d = col[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = k + 1 + (int)threadIdx.x + 256 * j;
        c[j] = i < m ? col[i] : 0.0;
    }
}

// R^T x = y over the leading m x m block of the factor A (column-major, leading dimension M); x overwrites v.  The column
// of the next step is fetched while this one is worked: the factor does not change here.
__device__ __forceinline__ void bss_back(const double* __restrict__ A, int M, int m, double* v, double* red) {
    const int tid = threadIdx.x;
    double cur[4], nxt[4] = {0.0, 0.0, 0.0, 0.0}, dcur, dnxt = 0.0;
    bss_column(A, M, m, m - 1, cur, dcur);
    for (int k = m - 1; k >= 0; --k) {
        if (k > 0) bss_column(A, M, m, k - 1, nxt, dnxt);
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = k + 1 + tid + 256 * j;
            if (i < m) a = __fma_rn(cur[j], v[i], a);
        }
        a = wave_sum(a);
        if ((tid & 63) == 0) red[tid >> 6] = a;
        __syncthreads();
        if (tid == 0) {
            const double s = __dadd_rn(__dadd_rn(__dadd_rn(red[0], red[1]), red[2]), red[3]);
            v[k] = __dsub_rn(v[k], s) / dcur;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
        dcur = dnxt;
    }
}

// One workgroup per clip.  The panel: kBssPanel = 16 columns of up to kBssMaxM = 1,024 rows in LDS, column-major, 16 x 1,024
// x 8 = 128 KiB of the CU's 160 KiB (a 64-column panel would be 512 KiB, a 20-column one all 160 KiB); with the two vectors
// of the solves (8 + 4 KiB) and the reduction's four doubles 143,392 bytes.  The trailing matrix stays in the workspace:
// thread l holds rows l, l + 256, l + 512, l + 768 below the panel -- their 4 x 16 panel values in registers -- and walks
// the trailing columns, whose 16 panel values are one LDS address per wavefront.
__global__ void __launch_bounds__(256) bss_chol_kernel(int L, int J, const double* __restrict__ lag, double* __restrict__ G,
                                                       double* __restrict__ sol, double* __restrict__ filt, int* __restrict__ flag) {
    __shared__ double pan[kBssPanel * kBssMaxM];
    __shared__ double v[kBssMaxM];
    __shared__ double v0[kBssMaxL];
    __shared__ double red[4];
    constexpr int NB = kBssPanel, LD = kBssMaxM;
    const int tid = threadIdx.x, M = J * L, NI = J == 2 ? 6 : 2;
    const size_t clip = blockIdx.x;
    const double* __restrict__ lg = lag + clip * NI * L;
    double* __restrict__ A = G + clip * M * M;
    double* __restrict__ out = sol + clip * (size_t)(M + L);
    double* __restrict__ fout = filt ? filt + clip * (size_t)(M + L) : nullptr;
    const double thr = __dmul_rn((double)M, 2.220446049250313e-16);      // J L 2^-52
    const double g00 = lg[0], g11 = J == 2 ? lg[3 * L] : 0.0;
    for (int k0 = 0; k0 < M; k0 += NB) {
        const int nb = M - k0 < NB ? M - k0 : NB, m = M - k0;
        for (int r = tid; r < m; r += 256) {        // (a row's loads issued together, then stored)
            double t[NB];
#pragma unroll
            for (int p = 0; p < NB; ++p) t[p] = p < nb && r >= p ? A[(size_t)(k0 + p) * M + k0 + r] : 0.0;
#pragma unroll
            for (int p = 0; p < NB; ++p)
                if (p < nb && r >= p) pan[p * LD + r] = t[p];
        }
        __syncthreads();
        for (int p = 0; p < nb; ++p) {
            const double piv = pan[p * LD + p];
            if (!(fabs(piv) <= 1.79769313486231570e308) || piv <= __dmul_rn(thr, k0 + p < L ? g00 : g11)) {
                // singular (the same value in every thread: the whole workgroup leaves)
                const double nan = quiet_nan();
                for (int i = tid; i < M + L; i += 256) { out[i] = nan; if (fout) fout[i] = nan; }
                if (tid == 0) flag[clip] = 1;
                return;
            }
            const double d = sqrt(piv);
            __syncthreads();
            for (int r = p + 1 + tid; r < m; r += 256) pan[p * LD + r] = pan[p * LD + r] / d;
            if (tid == 0) pan[p * LD + p] = d;
            __syncthreads();
            for (int q = p + 1; q < nb; ++q) {
                const double lq = pan[p * LD + q];
                for (int r = q + tid; r < m; r += 256) pan[q * LD + r] = __fma_rn(-pan[p * LD + r], lq, pan[q * LD + r]);
            }
            __syncthreads();
        }
        for (int p = 0; p < nb; ++p)
            for (int r = p + tid; r < m; r += 256) A[(size_t)(k0 + p) * M + k0 + r] = pan[p * LD + r];
        if (m > nb) {       // (nb == NB here: only the last panel is narrower, and nothing trails it)
            double li[4][NB];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = NB + tid + 256 * j;
#pragma unroll
                for (int p = 0; p < NB; ++p) li[j][p] = r < m ? pan[p * LD + r] : 0.0;
            }
            // four trailing columns at a time: their elements are fetched together, then each takes its chain
            for (int c0 = NB; c0 < m; c0 += 4) {
                double a[4][4];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const int c = c0 + cc;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = NB + tid + 256 * j;
                        a[cc][j] = c < m && r < m && r >= c ? A[(size_t)(k0 + c) * M + k0 + r] : 0.0;
                    }
                }
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const int c = c0 + cc;
                    if (c >= m) break;
                    double lc[NB];
#pragma unroll
                    for (int p = 0; p < NB; ++p) lc[p] = pan[p * LD + c];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = NB + tid + 256 * j;
                        if (r < m && r >= c) {
                            double x = a[cc][j];
#pragma unroll
                            for (int p = 0; p < NB; ++p) x = __fma_rn(-li[j][p], lc[p], x);
                            A[(size_t)(k0 + c) * M + k0 + r] = x;
                        }
                    }
                }
            }
        }
        __syncthreads();    // (the next panel reads what this workgroup has just stored)
    }
    // R y = D
    for (int i = tid; i < M; i += 256) v[i] = lg[(J == 2 ? 4 * L : L) + i];
    __syncthreads();
    {   // (the column of the next step is fetched while this one is worked)
        double cur[4], nxt[4] = {0.0, 0.0, 0.0, 0.0}, dcur, dnxt = 0.0;
        bss_column(A, M, M, 0, cur, dcur);
        for (int k = 0; k < M; ++k) {
            if (k + 1 < M) bss_column(A, M, M, k + 1, nxt, dnxt);
            const double yk = v[k] / dcur;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = k + 1 + tid + 256 * j;
                if (i < M) v[i] = __fma_rn(-cur[j], yk, v[i]);
            }
            if (tid == 0) v[k] = yk;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
            dcur = dnxt;
        }
    }
    if (J == 2) {
        for (int i = tid; i < L; i += 256) v0[i] = v[i];
        __syncthreads();
        bss_back(A, M, L, v0, red);
    }
    bss_back(A, M, M, v, red);
    for (int i = tid; i < M; i += 256) { out[i] = v[i]; if (fout) fout[i] = v[i]; }
    for (int i = tid; i < L; i += 256) {
        const double c0 = J == 2 ? v0[i] : v[i];
        out[M + i] = c0; if (fout) fout[M + i] = c0;
    }
    if (tid == 0) flag[clip] = 0;
}

// One workgroup: kBssProjTile samples t of one clip's [0, n + L - 1), four per thread.  Staged: the sources' samples
// [t0 - (L - 1), t0 + kBssProjTile) as doubles and the 3 L coefficients.
__global__ void __launch_bounds__(256) bss_project_kernel(const BssRun* __restrict__ runs, int nruns, int L, int J, const double* __restrict__ sol,
                                                          const int* __restrict__ flag, double* __restrict__ epart) {
    __shared__ double w[2][kBssProjWin];
    __shared__ double cf[3 * kBssMaxL];
    __shared__ double red[6][256];
    const int tid = threadIdx.x, M = J * L;
    const long long b = blockIdx.x;
    const int ri = find_run<BssRun, &BssRun::ptile0>(runs, nruns, b);
    if (flag[ri]) return;       // (the whole workgroup)
    const BssRun run = runs[ri];
    const long long t0 = (b - run.ptile0) * kBssProjTile, T = run.n + L - 1;
    const int W = kBssProjTile + L - 1;
    for (int i = tid; i < W; i += 256) {
        const long long t = t0 - (L - 1) + i;
        const bool ok = t >= 0 && t < run.n;
        w[0][i] = ok ? (double)run.s0[t] : 0.0;
        w[1][i] = ok && J == 2 ? (double)run.s1[t] : 0.0;
    }
    for (int i = tid; i < M + L; i += 256) cf[i] = sol[(size_t)ri * (M + L) + i];
    __syncthreads();
    const double* __restrict__ c0 = cf + M;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < kBssProjTile / 256; ++j) {
        const int tt = tid + 256 * j;
        const long long t = t0 + tt;
        if (t >= T) break;
        const double* __restrict__ x0 = w[0] + tt + (L - 1);
        const double* __restrict__ x1 = w[1] + tt + (L - 1);
        double P = 0.0, st = 0.0;
#pragma unroll 4
        for (int k = 0; k < L; ++k) {
            const double x = x0[-k];
            P = __fma_rn(cf[k], x, P);
            st = __fma_rn(c0[k], x, st);
        }
        if (J == 2) {
#pragma unroll 4
            for (int k = 0; k < L; ++k) P = __fma_rn(cf[L + k], x1[-k], P);
        }
        const double e = t < run.n ? (double)run.est[t] : 0.0;
        const double ei = __dsub_rn(P, st), ea = __dsub_rn(e, P), ed = __dsub_rn(e, st), ti = __dadd_rn(st, ei);
        acc[0] = __fma_rn(e, e, acc[0]); acc[1] = __fma_rn(st, st, acc[1]); acc[2] = __fma_rn(ei, ei, acc[2]);
        acc[3] = __fma_rn(ea, ea, acc[3]); acc[4] = __fma_rn(ed, ed, acc[4]); acc[5] = __fma_rn(ti, ti, acc[5]);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) red[q][tid] = acc[q];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int q = 0; q < 6; ++q) red[q][tid] = __dadd_rn(red[q][tid], red[q][tid + off]);
        }
        __syncthreads();
    }
    if (tid < 6) epart[(size_t)b * 6 + tid] = red[tid][0];
}

__device__ __forceinline__ double bss_db(double num, double den) { return __dmul_rn(10.0, log10(num / den)); }

// One wavefront per clip: the energies, the figures, the record.
__global__ void __launch_bounds__(64) bss_finish_kernel(const BssRun* __restrict__ runs, int L, int J, const int* __restrict__ flag,
                                                        const double* __restrict__ epart, double* __restrict__ rec) {
    __shared__ double E[6];
    const int tid = threadIdx.x;
    const BssRun run = runs[blockIdx.x];
    const bool bad = flag[blockIdx.x] != 0;
    if (tid < 6) {
        double a = 0.0;
        if (bad) a = quiet_nan();
        else for (long long k = 0; k < run.ptiles; ++k) a = __dadd_rn(a, epart[(size_t)(run.ptile0 + k) * 6 + tid]);
        E[tid] = a;
    }
    __syncthreads();
    double* __restrict__ o = rec + (size_t)blockIdx.x * kBssFields;
    if (tid < 6) o[3 + tid] = E[tid];
    if (tid == 6) { o[0] = (double)run.n; o[1] = (double)J; o[2] = (double)L; o[12] = bad ? 1.0 : 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 0.0; }
    // E: 0 E_e, 1 E_tgt, 2 E_int, 3 E_art, 4 E_dist, 5 E_ti
    if (tid == 7) o[9] = bad ? quiet_nan() : bss_db(E[1], E[4]);
    if (tid == 8) o[10] = bad ? quiet_nan() : bss_db(E[1], E[2]);
    if (tid == 9) o[11] = bad ? quiet_nan() : bss_db(E[5], E[3]);
}

}  // namespace

void launch_bss_corr(const char* kernel, const BssRun* runs_dev, int nruns, long long ntiles, int L, int J, double* part, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    if (L < 1 || L > kBssMaxL || J < 1 || J > 2) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, bss_corr_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, L, J, part);
}

void launch_bss_reduce(const char* kernel, const BssRun* runs_dev, int nruns, int L, int J, const double* part, double* lag, hipStream_t s) {
    if (nruns <= 0) return;
    if (L < 1 || L > kBssMaxL || J < 1 || J > 2) { note_refusal(kernel); return; }
    const int NIL = (J == 2 ? 6 : 2) * L;
    NHANS_LAUNCH(kernel, bss_reduce_kernel, dim3(nruns, (NIL + 255) / 256), dim3(256), 0, s, runs_dev, NIL, part, lag);
}

void launch_bss_gram(const char* kernel, int nruns, int L, int J, const double* lag, double* G, hipStream_t s) {
    if (nruns <= 0) return;
    if (L < 1 || L > kBssMaxL || J < 1 || J > 2) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, bss_gram_kernel, dim3(nruns, J * L), dim3(256), 0, s, L, J, lag, G);
}

void launch_bss_chol(const char* kernel, int nruns, int L, int J, const double* lag, double* G, double* sol, double* filt, int* flag,
                     hipStream_t s) {
    if (nruns <= 0) return;
    if (L < 1 || L > kBssMaxL || J < 1 || J > 2) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, bss_chol_kernel, dim3(nruns), dim3(256), 0, s, L, J, lag, G, sol, filt, flag);
}

void launch_bss_project(const char* kernel, const BssRun* runs_dev, int nruns, long long ntiles, int L, int J, const double* sol,
                        const int* flag, double* epart, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    if (L < 1 || L > kBssMaxL || J < 1 || J > 2) { note_refusal(kernel); return; }
    NHANS_LAUNCH(kernel, bss_project_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, L, J, sol, flag, epart);
}

void launch_bss_finish(const char* kernel, const BssRun* runs_dev, int nruns, int L, int J, const int* flag, const double* epart, double* rec,
                       hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, bss_finish_kernel, dim3(nruns), dim3(64), 0, s, runs_dev, L, J, flag, epart, rec);
}

}  // namespace nhans
