// Mixing speech with two noises at chosen SNRs on the device (include/nhans_hip.h: nhans_mix):
// the rule of n-hans_amd/mixing.py (domixing / domixing_separator), bit for bit.
//
// Float32 speech s of n samples, noises a (kept) and b (dropped) of ma, mb samples:
//     fit      A[i] = a[i mod ma] where ma < n, else a[i]  (i < n);  B likewise
//     power    sq[i] = float32(x[i] x[i]);  S = ((0.0 + double(sq[0])) + double(sq[1])) + ...  ONE dependent chain of
//              float64 additions in index order;  P = S / double(n)
//     gain     g = sqrt((P_s / P_noise) f) in double, f = pow(10, -snr_db / 10) from the HOST (a device pow may differ in
//              the last place);  g = 1 where P_noise == 0;  g32 = float32(g)
//     raw      raw[i] = (s[i] + g32a A[i]) + g32b B[i]: two float32 products and two float32 sums, each rounded on its own
//              (never contracted); without a keep noise raw[i] = s[i] + g32b B[i] -- nothing is added, not even zeros
//     finish   pk = max |raw|, p = float32(pk + 1e-6f), mixture = raw / p;  unit = float32(float32(pk / p) + 1e-6f) -- the
//              peak of the normalised mixture plus 1e-6 (the division is monotone) --, target = (s + g32a A) / unit,
//              keep = g32a A / unit, drop = g32b B / unit: the reference's quirk, divided by about 1 and not by p
//
// mix_power: one workgroup per DISTINCT (clip, fitted length).  The chain is the definition, so one lane adds; what the
// other lanes can do is keep it fed: waves 1 - 3 stage the next tile of kMixTile squares into one LDS buffer (the wrap
// resolved while staging) while lane 0 of wave 0 chains the current one out of the other.
// mix_combine, mix_finish: one workgroup per tile of kMixTile samples of a job.  Every workgroup of a job forms the
// job's gains from the three powers itself -- a division, a product and a square root in double, the same bits
// everywhere.  A maximum is exact in any order: per-tile peaks, then the maximum of a job's peaks in every workgroup of
// mix_finish.  No atomics.  Samples move through LDS: 16-byte loads and stores where the tile's address allows them,
// single ones for the head and tail (and for a noise that wraps), so an odd offset changes how a sample is fetched and
// nothing about what is computed.
#include "score_common.h"

namespace nhans {

namespace {

template <bool SQ>
__device__ __forceinline__ float staged(float v) { return SQ ? __fmul_rn(v, v) : v; }

// samples [s0, s0 + cnt) of the clip of m samples at src, fitted (wrap: sample i is src[i mod m]) -> dst (LDS), by threads
// t = 0 .. nt - 1 of the workgroup; SQ: their float32 squares
template <bool SQ>
__device__ __forceinline__ void stage_fit(const float* __restrict__ src, long long m, bool wrap, long long s0, int cnt, float* dst,
                                          int t, int nt) {
    if (wrap) {
        const long long start = s0 % m;
        for (int i = t; i < cnt; i += nt) dst[i] = staged<SQ>(src[(start + i) % m]);
        return;
    }
    const float* __restrict__ p = src + s0;
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
    if (head > cnt) head = cnt;
    const int n4 = (cnt - head) >> 2;
    if (t < head) dst[t] = staged<SQ>(p[t]);
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(p + head);
    for (int i = t; i < n4; i += nt) {
        const float4 v = v4[i];
        float* d = dst + head + 4 * i;
        d[0] = staged<SQ>(v.x); d[1] = staged<SQ>(v.y); d[2] = staged<SQ>(v.z); d[3] = staged<SQ>(v.w);
    }
    const int done = head + 4 * n4;
    if (t < cnt - done) dst[done + t] = staged<SQ>(p[done + t]);
}

// cnt <= kMixTile samples of src (LDS) -> dst, by the whole workgroup
__device__ __forceinline__ void store_tile(float* __restrict__ dst, const float* src, int cnt, int tid) {
    int head = (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3);
    if (head > cnt) head = cnt;
    const int n4 = (cnt - head) >> 2;
    if (tid < head) dst[tid] = src[tid];
    float4* __restrict__ v4 = reinterpret_cast<float4*>(dst + head);
    for (int i = tid; i < n4; i += 256) {
        const float* s = src + head + 4 * i;
        v4[i] = make_float4(s[0], s[1], s[2], s[3]);
    }
    const int done = head + 4 * n4;
    if (tid < cnt - done) dst[done + tid] = src[done + tid];
}

// the maximum over the workgroup, in every thread
__device__ __forceinline__ float block_max(float v, float* w, int tid) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off));
    if ((tid & 63) == 0) w[tid >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
    __syncthreads();
    return v;
}

// One workgroup per chain: pw[chain] = (the chain of the fitted clip's float32 squares) / n.
__global__ void __launch_bounds__(256) mix_power_kernel(const MixChain* __restrict__ chains, double* __restrict__ pw) {
    __shared__ float sq[2][kMixTile];
    const int tid = threadIdx.x;
    const MixChain c = chains[blockIdx.x];
    const bool wrap = c.m < c.n, stager = tid >= 64;
    const long long nt = (c.n + kMixTile - 1) / kMixTile;
    const int last = (int)(c.n - (nt - 1) * kMixTile);
    if (stager) stage_fit<true>(c.src, c.m, wrap, 0, nt == 1 ? last : kMixTile, sq[0], tid - 64, 192);
    __syncthreads();
    double S = 0.0;
    for (long long t = 0; t < nt; ++t) {
        if (stager) {
            if (t + 1 < nt)
                stage_fit<true>(c.src, c.m, wrap, (t + 1) * kMixTile, t + 2 == nt ? last : kMixTile, sq[(t + 1) & 1], tid - 64, 192);
        } else if (tid == 0) {
            // (unrolled: the LDS reads of eight squares are in flight while the one chain of additions runs)
            const float* b = sq[t & 1];
            const int cnt = t + 1 == nt ? last : kMixTile;
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) S = __dadd_rn(S, (double)b[j]);
        }
        __syncthreads();
    }
    if (tid == 0) pw[blockIdx.x] = S / (double)c.n;
}

__device__ __forceinline__ double snr_gain(double p_speech, double p_noise, double f) {
    return p_noise == 0.0 ? 1.0 : sqrt(__dmul_rn(p_speech / p_noise, f));
}

// the three signals of a tile in LDS and the job's gains
struct MixTile {
    const MixJob& job;
    const float *ss, *sa, *sb;
    float ga, gb;
    // (products and sums rounded one by one, as mix_sample of resample.hip: DESIGN.md section 1.5)
    __device__ __forceinline__ float kept(int i) const {
#pragma clang fp contract(off)
        const float p = ga * sa[i];
        return p;
    }
    __device__ __forceinline__ float dropped(int i) const {
#pragma clang fp contract(off)
        const float p = gb * sb[i];
        return p;
    }
    // speech plus the kept noise: the speech itself in the two-way mix
    __device__ __forceinline__ float wanted(int i) const {
#pragma clang fp contract(off)
        if (!job.a) return ss[i];
        const float p = kept(i);
        return ss[i] + p;
    }
    __device__ __forceinline__ float raw(int i) const {
#pragma clang fp contract(off)
        const float w = wanted(i), p = dropped(i);
        return w + p;
    }
};

__device__ __forceinline__ void stage_job(const MixJob& job, long long s0, int cnt, float* ss, float* sa, float* sb, int tid) {
    stage_fit<false>(job.s, job.n, false, s0, cnt, ss, tid, 256);
    if (job.a) stage_fit<false>(job.a, job.ma, job.ma < job.n, s0, cnt, sa, tid, 256);
    stage_fit<false>(job.b, job.mb, job.mb < job.n, s0, cnt, sb, tid, 256);
}

// One workgroup per tile: raw -> mixture, max |raw| -> peaks[tile]; a job's first tile: fields 0 - 4 of its record.
__global__ void __launch_bounds__(256) mix_combine_kernel(const MixJob* __restrict__ jobs, int njobs, const double* __restrict__ pw,
                                                          float* __restrict__ mixture, float* __restrict__ peaks,
                                                          double* __restrict__ rec) {
    __shared__ float ss[kMixTile], sa[kMixTile], sb[kMixTile], wmax[4];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const int ji = find_run<MixJob, &MixJob::tile0>(jobs, njobs, b);
    const MixJob job = jobs[ji];
    const long long s0 = (b - job.tile0) * kMixTile, left = job.n - s0;
    const int cnt = (int)(left < kMixTile ? left : kMixTile);
    stage_job(job, s0, cnt, ss, sa, sb, tid);
    const double Ps = pw[job.ps], Pa = job.a ? pw[job.pa] : 0.0, Pb = pw[job.pb];
    const double ga = job.a ? snr_gain(Ps, Pa, job.fa) : 1.0, gb = snr_gain(Ps, Pb, job.fb);
    if (rec && s0 == 0 && tid == 0) {
        double* o = rec + (size_t)ji * kMixFields;
        o[0] = Ps; o[1] = Pa; o[2] = Pb; o[3] = ga; o[4] = gb;
    }
    __syncthreads();
    const MixTile t{job, ss, sa, sb, (float)ga, (float)gb};
    float m = 0.f;
    for (int i = tid; i < cnt; i += 256) {
        const float r = t.raw(i);
        ss[i] = r;                      // (read and written by this thread alone)
        m = fmaxf(m, fabsf(r));
    }
    m = block_max(m, wmax, tid);
    store_tile(mixture + job.out + s0, ss, cnt, tid);
    if (tid == 0) peaks[b] = m;
}

// One workgroup per tile: the mixture divided in place, the three other signals where asked for; a job's first tile:
// fields 5 - 7 of its record.
__global__ void __launch_bounds__(256) mix_finish_kernel(const MixJob* __restrict__ jobs, int njobs, const double* __restrict__ pw,
                                                         const float* __restrict__ peaks, float* mixture, float* __restrict__ target,
                                                         float* __restrict__ keep, float* __restrict__ drop, double* __restrict__ rec) {
    __shared__ float ss[kMixTile], sa[kMixTile], sb[kMixTile], so[kMixTile], wmax[4];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const int ji = find_run<MixJob, &MixJob::tile0>(jobs, njobs, b);
    const MixJob job = jobs[ji];
    const long long s0 = (b - job.tile0) * kMixTile, left = job.n - s0;
    const int cnt = (int)(left < kMixTile ? left : kMixTile);
    const long long ntiles = (job.n + kMixTile - 1) / kMixTile;
    stage_job(job, s0, cnt, ss, sa, sb, tid);
    stage_fit<false>(mixture + job.out, job.n, false, s0, cnt, so, tid, 256);
    float pk = 0.f;
    for (long long i = tid; i < ntiles; i += 256) pk = fmaxf(pk, peaks[job.tile0 + i]);
    pk = block_max(pk, wmax, tid);      // (its barriers also publish the staged tiles)
    const float p = __fadd_rn(pk, 1e-6f), unit = __fadd_rn(__fdiv_rn(pk, p), 1e-6f);
    const double Ps = pw[job.ps];
    const MixTile t{job, ss, sa, sb, job.a ? (float)snr_gain(Ps, pw[job.pa], job.fa) : 1.f, (float)snr_gain(Ps, pw[job.pb], job.fb)};
    if (rec && s0 == 0 && tid == 0) {
        double* o = rec + (size_t)ji * kMixFields;
        o[5] = (double)pk; o[6] = (double)unit; o[7] = 0.0;
    }
    const size_t at = (size_t)(job.out + s0);
    for (int i = tid; i < cnt; i += 256) so[i] = __fdiv_rn(so[i], p);
    __syncthreads();
    store_tile(mixture + at, so, cnt, tid);
    if (target) {
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) so[i] = __fdiv_rn(t.wanted(i), unit);
        __syncthreads();
        store_tile(target + at, so, cnt, tid);
    }
    if (keep) {         // (the two-way mix keeps nothing: zeros)
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) so[i] = job.a ? __fdiv_rn(t.kept(i), unit) : 0.f;
        __syncthreads();
        store_tile(keep + at, so, cnt, tid);
    }
    if (drop) {
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) so[i] = __fdiv_rn(t.dropped(i), unit);
        __syncthreads();
        store_tile(drop + at, so, cnt, tid);
    }
}

}  // namespace

void launch_mix_power(const char* kernel, const MixChain* chains_dev, int nchains, double* pw, hipStream_t s) {
    if (nchains <= 0) return;
    NHANS_LAUNCH(kernel, mix_power_kernel, dim3(nchains), dim3(256), 0, s, chains_dev, pw);
}

void launch_mix_combine(const char* kernel, const MixJob* jobs_dev, int njobs, long long ntiles, const double* pw, float* mixture,
                        float* peaks, double* rec, hipStream_t s) {
    if (!tiles_ok(kernel, njobs, ntiles)) return;
    NHANS_LAUNCH(kernel, mix_combine_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, jobs_dev, njobs, pw, mixture, peaks, rec);
}

void launch_mix_finish(const char* kernel, const MixJob* jobs_dev, int njobs, long long ntiles, const double* pw, const float* peaks,
                       float* mixture, float* target, float* keep, float* drop, double* rec, hipStream_t s) {
    if (!tiles_ok(kernel, njobs, ntiles)) return;
    NHANS_LAUNCH(kernel, mix_finish_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, jobs_dev, njobs, pw, peaks, mixture, target, keep,
                 drop, rec);
}

}  // namespace nhans
