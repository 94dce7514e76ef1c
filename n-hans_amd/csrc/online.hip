// Data movement of online enhancement (nhans_online_push, host_online.hip): carried samples + new input -> the STFT's
// staging buffer, history rows of the state + the push's new rows -> the window source of the stack, synthesis staging
// for the iSTFT, final samples -> the caller, and the next state slot.  Every move is a list of contiguous runs built on
// the host; one launch per list, one workgroup per run.  Pure copies: the bits are those of the kernels that made them.
// capture_clip_kernel (nhans_capture_context): a slot's ring of its last kCaptureSamples 16 kHz samples -> a linear
// context clip, optionally through the arithmetic of peak_normalise_kernel (resample.hip).
#include "nhans_kernels.h"

namespace nhans {

__global__ void __launch_bounds__(256) online_copy_kernel(const OnlineCopy* __restrict__ runs) {
    const OnlineCopy r = runs[blockIdx.x];
    const int n = (int)r.n;
    for (int i = threadIdx.x; i < n; i += 256) r.dst[i] = r.src[i];
}

// One workgroup per entry.  Chronological sample j of the clip is ring[(start + j) mod kCaptureSamples]: two contiguous
// spans, [start, kCaptureSamples) then [0, start).  normalise: out = float32(double(x) / (double(max|x|) + 1e-6)) -- max is
// exact, so the reduction tree does not matter and the bits are those of peak_partial_kernel + peak_normalise_kernel.
__global__ void __launch_bounds__(kCaptureThreads) capture_clip_kernel(const CaptureEntry* __restrict__ entries) {
    __shared__ float part[kCaptureThreads / 64];
    const CaptureEntry e = entries[blockIdx.x];
    const int first = kCaptureSamples - e.start;       // samples [0, first) sit at ring + start, the rest at ring + 0
    double den = 1.0;
    if (e.normalise) {
        float m = -INFINITY;
        for (int j = threadIdx.x; j < kCaptureSamples; j += kCaptureThreads)
            m = fmaxf(m, fabsf(e.ring[j < first ? e.start + j : j - first]));
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
        __syncthreads();
        m = part[0];
        for (int w = 1; w < kCaptureThreads / 64; ++w) m = fmaxf(m, part[w]);
        den = (double)m + 0.000001;
    }
    for (int j = threadIdx.x; j < kCaptureSamples; j += kCaptureThreads) {
        const float v = e.ring[j < first ? e.start + j : j - first];
        e.clip[j] = e.normalise ? (float)((double)v / den) : v;
    }
}

void launch_capture_clip(const CaptureEntry* entries_dev, int n, hipStream_t s) {
    if (n <= 0) return;
    NHANS_LAUNCH("capture_clip_kernel", capture_clip_kernel, dim3(n), dim3(kCaptureThreads), 0, s, entries_dev);
}

void launch_online_copy(const char* kernel, const OnlineCopy* runs_dev, int nruns, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, online_copy_kernel, dim3(nruns), dim3(256), 0, s, runs_dev);
}

}  // namespace nhans
