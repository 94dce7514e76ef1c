// Filterbank features of log-magnitude rows (include/nhans_hip.h: nhans_fbank_*).
//
// For a row x[201] (float32, natural log) and a filterbank of n_out bands -- band m: non-negative float32 weights over
// the bins [first_m, first_m + count_m) -- output m is
//     p[k] = expf(power * x[k]),   mel = sum_k w[m][k] p[k],   out[m] = logf(max(mel, floor)),
// the sum ONE chain of count_m fmaf in float32 from +0.0f, k ascending (fbank_out below, the fir_chain idiom of
// resample.hip), so a row's bits depend on the row and the filterbank only: the offline call and the launch inside an
// online push run this one kernel body on run descriptors, and where a row sits in a run, a tile or a launch only
// changes where it is fetched from and stored to.
//
// One workgroup = one tile of kFbankTile consecutive rows of one run.  It copies the band table into LDS (per band
// first, count and the offset of its weights; the weights contiguous), stages p ONCE per (row, bin) -- 201 expf per row,
// not one per tap; the rows fetched in 16-byte pieces where the run is aligned: 0.108 -> 0.087 ms per 255,488 rows --, then its threads walk the tile's (row, band) outputs with the band index fastest: the stores of a
// wavefront are contiguous, and a wavefront's LDS reads of p stay within a few rows (row stride 201 floats, odd: the
// same bin of neighbouring rows is in different banks).  LDS: 12,864 B of p plus the table, 4.8 KB for an 80-band mel
// bank and at most 34.3 KB (kFbankMaxSpan weights), so at least three and usually eight workgroups share a CU.
#include "nhans_kernels.h"

namespace nhans {

namespace {

// p of one bin.  power * x is exact for power 1 and 2; the clamp keeps p a finite float32 for rows outside the domain
// of the network's rows (expf(88) = 1.65e38) and changes nothing inside it.
__device__ __forceinline__ float fbank_power(float x, int power) {
    const float a = power == 2 ? x + x : x;
    return expf(fminf(a, kFbankMaxExponent));
}

// The one accumulation and logarithm every filterbank output of the library goes through: weights w[0 .. cnt) and the
// powers of the band's bins p[0 .. cnt), both in LDS.  An empty band (cnt == 0) gives logf(floor).
__device__ __forceinline__ float fbank_out(const float* w, const float* p, int cnt, float floor) {
    float acc = 0.f;
    for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], p[j], acc);
    return logf(fmaxf(acc, floor));
}

__global__ void __launch_bounds__(256) fbank_kernel(const FbankRun* __restrict__ runs, int nruns, const int* __restrict__ table,
                                                    int n_out, int nwords, int power, float floor) {
    extern __shared__ int fb_lds[];
    const int* first = fb_lds;
    const int* count = fb_lds + n_out;
    const int* woff = fb_lds + 2 * n_out;
    const float* wt = reinterpret_cast<const float*>(fb_lds + 3 * n_out);
    float* p = reinterpret_cast<float*>(fb_lds + nwords);
    const int tid = threadIdx.x;
    for (int i = tid; i < nwords; i += 256) fb_lds[i] = table[i];
    // the run this tile belongs to (tile0 ascending; a launch has a handful of runs)
    const long long b = blockIdx.x;
    int r = 0;
    while (r + 1 < nruns && runs[r + 1].tile0 <= b) ++r;
    const FbankRun run = runs[r];
    const long long row0 = (b - run.tile0) * kFbankTile;
    const long long left = run.nrows - row0;
    const int nr = (int)(left < kFbankTile ? left : kFbankTile);
    const float* __restrict__ src = run.src + row0 * kBins;
    // (a tile is 12,864 B from a multiple of 12,864 B: 16-byte pieces wherever the run itself starts on one; the same
    // function on the same values either way)
    const int n = nr * kBins;
    const int n4 = (reinterpret_cast<uintptr_t>(run.src) & 15) == 0 ? n >> 2 : 0;
    for (int i = tid; i < n4; i += 256) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        p[4 * i + 0] = fbank_power(v.x, power); p[4 * i + 1] = fbank_power(v.y, power);
        p[4 * i + 2] = fbank_power(v.z, power); p[4 * i + 3] = fbank_power(v.w, power);
    }
    for (int i = 4 * n4 + tid; i < n; i += 256) p[i] = fbank_power(src[i], power);
    __syncthreads();
    float* __restrict__ dst = run.dst + row0 * n_out;
    for (int o = tid; o < nr * n_out; o += 256) {
        const int row = o / n_out, m = o - row * n_out;
        dst[o] = fbank_out(wt + woff[m], p + row * kBins + first[m], count[m], floor);
    }
}

}  // namespace

size_t fbank_lds_bytes(int n_out, int nspan) { return ((size_t)3 * n_out + nspan + (size_t)kFbankTile * kBins) * 4; }

void launch_fbank(const char* kernel, const FbankRun* runs_dev, int nruns, long long ntiles, const int* table_dev, int n_out,
                  int nspan, int power, float floor, hipStream_t s) {
    if (nruns <= 0 || ntiles <= 0) return;
    if (ntiles > 0x7fffffffLL || n_out < 1 || n_out > kFbankMaxOut || nspan < 0 || nspan > kFbankMaxSpan) {
        note_refusal(kernel);
        return;
    }
    NHANS_LAUNCH(kernel, fbank_kernel, dim3((unsigned)ntiles), dim3(256), fbank_lds_bytes(n_out, nspan), s, runs_dev, nruns,
                 table_dev, n_out, 3 * n_out + nspan, power, floor);
}

}  // namespace nhans
