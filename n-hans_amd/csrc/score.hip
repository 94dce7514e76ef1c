// Scoring an estimate against a clean target on the device (include/nhans_hip.h: nhans_score_*).
//
// Waveform figures of an estimate e and a target t, float32, n common samples, every operation in double (a product of
// two float32 is exact in double):
//     See = sum e^2,  Stt = sum t^2,  Set = sum e t,  Sdd = sum (e - t)^2,
//     snr_db    = 10 log10(Stt / Sdd),
//     alpha     = Set / Stt,   r = fma(-alpha, t, e),   Srr = sum r^2   (a SECOND pass over the samples: the expanded
//                 form See - 2 alpha Set + alpha^2 Stt cancels when e ~ t),
//     si_sdr_db = 10 log10((alpha alpha) Stt / Srr)     (e bit-equal to t: alpha == 1, Srr == 0, +inf),
//     segsnr_db = the mean, over the frames f < nhans_num_frames(n) whose Pt != 0, of
//                 seg_f = clamp(10 log10(Pt / Pd), -10, 35),  Pt / Pd = sum t^2 / sum (e - t)^2 over samples
//                 [160 f, 160 f + 400);  Pd == 0: 35;  Pt == 0: the frame is skipped and counted as such.
//     Stt == 0 (n == 0 included): alpha = 0 and both dB figures NaN; no counted frame: segsnr_db NaN; non-finite samples
//     propagate (the clamp is two comparisons, which keep a NaN).
// Row figures of two [frames, 201] float32 log-magnitude tensors E and T, d = double(E) - double(T):
//     loss_f = (sum_k d^2 imp[k]) / 201,  imp = float32 linspace(2, 1, 201)          (the reference's loss, main.py:245-248)
//     lsd_f  = sqrt((sum_k ((20 / ln 10) d)^2) / 201),
//     loss, lsd_db = the mean over the clip's frames (no frame: NaN).
//
// The order of every sum is fixed relative to the clip's first sample, so a figure's bits are a property of the clip pair
// -- not of its place in the batch, its neighbours, the alignment of its first sample or the run:
//   * a clip is cut into SEGMENTS of 80 samples (the greatest common divisor of the 400-sample frame and its 160-sample
//     hop) from its first sample on, the last one shorter.  Sixteen lanes sum a segment: lane l adds its terms of samples
//     l, l + 16, ..., l + 64 of the segment in that order (one __fma_rn from +0.0 each), then the __shfl_down tree 8, 4, 2,
//     1 in __dadd_rn;
//   * a TILE is 32 consecutive segments (2,560 samples), one workgroup: a tile's sum is its segments' sums added one
//     after the other in ascending order, a clip's sum its tiles' partials added one after the other in ascending order
//     (score_finish, one workgroup per clip, through LDS in rounds of 256);
//   * a frame's power is its five segments 2 f ... 2 f + 4 added in ascending order; the segmental mean adds the counted
//     frames' values one after the other in ascending frame order and divides once;
//   * a row's sums: lane k of one wavefront adds bins k, k + 64, k + 128, k + 192 in that order, then the __shfl_down tree
//     32, ..., 1; the clip's means add the rows' values one after the other in ascending frame order.
// No floating-point atomics, and no reduction whose shape depends on the batch.  The samples of a tile come in through
// LDS: 16-byte loads where the tile's address allows them and single loads for the head and tail where it does not, so
// an odd offset changes how a sample is fetched and nothing about where it is added.
#include "score_common.h"

namespace nhans {

namespace {

constexpr int kSeg = kScoreSegment, kSegsPerTile = kScoreTile / kScoreSegment;      // 80, 32

// sum over the 16 lanes of a segment's group; the group's first lane holds it
__device__ __forceinline__ double group_sum(double v) {
    for (int off = 8; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off, 16));
    return v;
}

// cnt <= kScoreTile samples at src -> dst (LDS), by the whole workgroup
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, int cnt, float* dst, int tid) {
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(src) >> 2) & 3)) & 3);
    if (head > cnt) head = cnt;
    const int n4 = (cnt - head) >> 2;
    if (tid < head) dst[tid] = src[tid];
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(src + head);
    for (int i = tid; i < n4; i += 256) {
        const float4 v = v4[i];
        float* d = dst + head + 4 * i;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    const int done = head + 4 * n4;
    if (tid < cnt - done) dst[done + tid] = src[done + tid];
}

// PASS 1: See, Stt, Set, Sdd of a tile -> part[tile][4], and Pt, Pd of its segments -> segs[segment][2].
// PASS 2: Srr of a tile -> part[tile][0], alpha read from the clip's record.
template <int PASS>
__global__ void __launch_bounds__(256) score_tiles_kernel(const ScoreRun* __restrict__ runs, int nruns, double* __restrict__ part,
                                                          double* __restrict__ segs, const double* __restrict__ rec) {
    __shared__ float se[kScoreTile], st[kScoreTile];
    __shared__ double sums[4][kSegsPerTile];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const int ri = find_run<ScoreRun, &ScoreRun::tile0>(runs, nruns, b);
    const ScoreRun run = runs[ri];
    const long long s0 = (b - run.tile0) * kScoreTile;
    const long long left = run.n - s0;
    const int cnt = (int)(left < kScoreTile ? left : kScoreTile);
    stage_tile(run.est + s0, cnt, se, tid);
    stage_tile(run.tgt + s0, cnt, st, tid);
    __syncthreads();
    const double nalpha = PASS == 2 ? -rec[(size_t)ri * kScoreFields + 5] : 0.0;
    const int g = tid >> 4, l = tid & 15;
    for (int round = 0; round < kSegsPerTile / 16; ++round) {
        const int seg = round * 16 + g, base = seg * kSeg;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int j = 0; j < kSeg / 16; ++j) {
            const int k = base + l + 16 * j;
            if (k < cnt) {
                const double e = (double)se[k], t = (double)st[k];
                if (PASS == 1) {
                    const double d = __dsub_rn(e, t);
                    a0 = __fma_rn(e, e, a0);
                    a1 = __fma_rn(t, t, a1);
                    a2 = __fma_rn(e, t, a2);
                    a3 = __fma_rn(d, d, a3);
                } else {
                    const double r = __fma_rn(nalpha, t, e);
                    a0 = __fma_rn(r, r, a0);
                }
            }
        }
        a0 = group_sum(a0);
        if (PASS == 1) { a1 = group_sum(a1); a2 = group_sum(a2); a3 = group_sum(a3); }
        if (l == 0) {
            sums[0][seg] = a0;
            if (PASS == 1) {
                sums[1][seg] = a1; sums[2][seg] = a2; sums[3][seg] = a3;
                if (base < cnt) {
                    double* o = segs + 2 * (size_t)(run.seg0 + (b - run.tile0) * kSegsPerTile + seg);
                    o[0] = a1; o[1] = a3;
                }
            }
        }
    }
    __syncthreads();
    if (tid < (PASS == 1 ? 4 : 1)) {
        double a = 0.0;
        for (int s = 0; s < kSegsPerTile; ++s) a = __dadd_rn(a, sums[tid][s]);      // (a segment past the end holds +0.0)
        part[(size_t)b * 4 + tid] = a;
    }
}

__device__ __forceinline__ double ten_log10(double q) { return __dmul_rn(10.0, log10(q)); }

// the running sum of nq quantities over the clip's tile partials, ascending, by threads 0 .. nq - 1 (the result is theirs)
__device__ __forceinline__ double tile_total(const double* __restrict__ part, long long tile0, long long ntiles, int nq,
                                             double (*buf)[256], int tid) {
    double a = 0.0;
    for (long long tb = 0; tb < ntiles; tb += 256) {
        const int nb = (int)(ntiles - tb < 256 ? ntiles - tb : 256);
        if (tid < nb)
            for (int q = 0; q < nq; ++q) buf[q][tid] = part[(size_t)(tile0 + tb + tid) * 4 + q];
        __syncthreads();
        if (tid < nq) {
#pragma unroll 8
            for (int j = 0; j < nb; ++j) a = __dadd_rn(a, buf[tid][j]);
        }
        __syncthreads();
    }
    return a;
}

// One workgroup per clip: the four sums, alpha, snr_db, the frames and the segmental mean.
__global__ void __launch_bounds__(256) score_finish_kernel(const ScoreRun* __restrict__ runs, const double* __restrict__ part,
                                                           const double* __restrict__ segs, double* __restrict__ rec,
                                                           double* __restrict__ frames_out) {
    __shared__ double buf[4][256];
    __shared__ double tot[4];
    const int tid = threadIdx.x;
    const ScoreRun run = runs[blockIdx.x];
    const long long ntiles = (run.n + kScoreTile - 1) / kScoreTile;
    const double a = tile_total(part, run.tile0, ntiles, 4, buf, tid);
    if (tid < 4) tot[tid] = a;
    __syncthreads();
    // the frames, 256 per round: thread t the value of frame fb + t, thread 0 the running sum
    double seg_sum = 0.0;
    long long skipped = 0;
    for (long long fb = 0; fb < run.frames; fb += 256) {
        const int nb = (int)(run.frames - fb < 256 ? run.frames - fb : 256);
        if (tid < nb) {
            const double* p = segs + 2 * (size_t)(run.seg0 + 2 * (fb + tid));
            double pt = p[0], pd = p[1];
            for (int j = 1; j < 5; ++j) { pt = __dadd_rn(pt, p[2 * j]); pd = __dadd_rn(pd, p[2 * j + 1]); }
            double v;
            bool skip = false;
            if (pt == 0.0) { skip = true; v = quiet_nan(); }
            else if (pd == 0.0) v = 35.0;
            else {
                v = ten_log10(pt / pd);
                v = v < -10.0 ? -10.0 : (v > 35.0 ? 35.0 : v);
            }
            buf[0][tid] = v;
            buf[1][tid] = skip ? 1.0 : 0.0;
            if (frames_out) frames_out[3 * (size_t)(run.frame0 + fb + tid)] = v;
        }
        __syncthreads();
        if (tid == 0) {
            // (a select, not a branch, and unrolled: the LDS reads of eight frames are in flight while one chain of additions runs)
#pragma unroll 8
            for (int j = 0; j < nb; ++j) {
                const double v = buf[0][j];
                const bool skip = buf[1][j] != 0.0;
                const double next = __dadd_rn(seg_sum, v);
                seg_sum = skip ? seg_sum : next;
                skipped += skip ? 1 : 0;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double nan = quiet_nan();
        const long long counted = run.frames - skipped;
        const double See = tot[0], Stt = tot[1], Set = tot[2], Sdd = tot[3];
        double* o = rec + (size_t)blockIdx.x * kScoreFields;
        o[0] = (double)run.n; o[1] = See; o[2] = Stt; o[3] = Set; o[4] = Sdd;
        o[5] = Stt == 0.0 ? 0.0 : Set / Stt;
        o[6] = 0.0;
        o[7] = Stt == 0.0 ? nan : ten_log10(Stt / Sdd);
        o[8] = nan;
        o[9] = counted > 0 ? seg_sum / (double)counted : nan;
        o[10] = (double)counted; o[11] = (double)skipped;
        o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
    }
}

// One workgroup per clip: Srr from the second pass's partials, then si_sdr_db.
__global__ void __launch_bounds__(256) score_sisdr_kernel(const ScoreRun* __restrict__ runs, const double* __restrict__ part,
                                                          double* __restrict__ rec) {
    __shared__ double buf[1][256];
    const int tid = threadIdx.x;
    const ScoreRun run = runs[blockIdx.x];
    const long long ntiles = (run.n + kScoreTile - 1) / kScoreTile;
    const double Srr = tile_total(part, run.tile0, ntiles, 1, buf, tid);
    if (tid == 0) {
        double* o = rec + (size_t)blockIdx.x * kScoreFields;
        const double alpha = o[5], Stt = o[2];
        o[6] = Srr;
        if (Stt != 0.0) o[8] = ten_log10(__dmul_rn(__dmul_rn(alpha, alpha), Stt) / Srr);
    }
}

// float32 linspace(2, 1, 201)[k] as numpy forms it: k * step + 2 in double, step = -1 / 200, two roundings; the end exact
__device__ __forceinline__ double score_imp(int k) {
    return k == kBins - 1 ? 1.0 : (double)(float)__dadd_rn(__dmul_rn((double)k, -0.005), 2.0);
}

// One workgroup: kScoreRowTile consecutive rows of one run, a wavefront per row in turn -> vals[row][2] = loss_f, lsd_f
// (and columns 1 - 2 of frames_out).
__global__ void __launch_bounds__(256) score_rows_kernel(const ScoreRowRun* __restrict__ runs, int nruns, double* __restrict__ vals,
                                                         double* __restrict__ frames_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    const int ri = find_run<ScoreRowRun, &ScoreRowRun::tile0>(runs, nruns, b);
    const ScoreRowRun run = runs[ri];
    const long long row0 = (b - run.tile0) * kScoreRowTile;
    const long long left = run.frames - row0;
    const int nr = (int)(left < kScoreRowTile ? left : kScoreRowTile);
    double imp[4];
    for (int j = 0; j < 4; ++j) imp[j] = score_imp(lane + 64 * j < kBins ? lane + 64 * j : 0);
    const double c = 20.0 / 2.302585092994046;      // 20 / ln 10 (8.685889638065035)
    for (int r = wave; r < nr; r += 4) {
        const float* __restrict__ e = run.est + (row0 + r) * kBins;
        const float* __restrict__ t = run.tgt + (row0 + r) * kBins;
        double al = 0.0, as = 0.0;
        for (int j = 0; j < 4; ++j) {
            const int k = lane + 64 * j;
            if (k < kBins) {
                const double d = __dsub_rn((double)e[k], (double)t[k]);
                al = __fma_rn(__dmul_rn(d, d), imp[j], al);
                const double cd = __dmul_rn(c, d);
                as = __fma_rn(cd, cd, as);
            }
        }
        al = wave_sum(al); as = wave_sum(as);
        if (lane == 0) {
            const double loss = al / (double)kBins, lsd = sqrt(as / (double)kBins);
            const size_t f = (size_t)(run.frame0 + row0 + r);
            vals[2 * f] = loss; vals[2 * f + 1] = lsd;
            if (frames_out) { frames_out[3 * f + 1] = loss; frames_out[3 * f + 2] = lsd; }
        }
    }
}

// One workgroup per clip: the means of its rows' values, ascending.
__global__ void __launch_bounds__(256) score_rows_finish_kernel(const ScoreRowRun* __restrict__ runs, const double* __restrict__ vals,
                                                                double* __restrict__ rec) {
    __shared__ double buf[2][256];
    const int tid = threadIdx.x;
    const ScoreRowRun run = runs[blockIdx.x];
    double a = 0.0;
    for (long long fb = 0; fb < run.frames; fb += 256) {
        const int nb = (int)(run.frames - fb < 256 ? run.frames - fb : 256);
        if (tid < nb) {
            const size_t f = (size_t)(run.frame0 + fb + tid);
            buf[0][tid] = vals[2 * f]; buf[1][tid] = vals[2 * f + 1];
        }
        __syncthreads();
        if (tid < 2) {
#pragma unroll 8
            for (int j = 0; j < nb; ++j) a = __dadd_rn(a, buf[tid][j]);
        }
        __syncthreads();
    }
    double* o = rec + (size_t)blockIdx.x * kScoreRowFields;
    const double nan = quiet_nan();
    if (tid < 2) o[1 + tid] = run.frames > 0 ? a / (double)run.frames : nan;
    if (tid == 2) o[0] = (double)run.frames;
    if (tid >= 3 && tid < kScoreRowFields) o[tid] = 0.0;
}

}  // namespace

void launch_score_tiles(const char* kernel, int pass, const ScoreRun* runs_dev, int nruns, long long ntiles, double* part,
                        double* segs, const double* rec, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    if (pass == 1)
        NHANS_LAUNCH(kernel, score_tiles_kernel<1>, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, part, segs, rec);
    else
        NHANS_LAUNCH(kernel, score_tiles_kernel<2>, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, part, segs, rec);
}

void launch_score_finish(const char* kernel, const ScoreRun* runs_dev, int nruns, const double* part, const double* segs,
                         double* rec, double* frames_out, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, score_finish_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, part, segs, rec, frames_out);
}

void launch_score_sisdr(const char* kernel, const ScoreRun* runs_dev, int nruns, const double* part, double* rec, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, score_sisdr_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, part, rec);
}

void launch_score_rows(const char* kernel, const ScoreRowRun* runs_dev, int nruns, long long ntiles, double* vals,
                       double* frames_out, hipStream_t s) {
    if (!tiles_ok(kernel, nruns, ntiles)) return;
    NHANS_LAUNCH(kernel, score_rows_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, runs_dev, nruns, vals, frames_out);
}

void launch_score_rows_finish(const char* kernel, const ScoreRowRun* runs_dev, int nruns, const double* vals, double* rec,
                              hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, score_rows_finish_kernel, dim3(nruns), dim3(256), 0, s, runs_dev, vals, rec);
}

}  // namespace nhans
