// Data movement of online enhancement (nhans_online_push, nhans_api.hip): carried samples + new input -> the STFT's
// staging buffer, history rows of the state + the push's new rows -> the window source of the stack, synthesis staging
// for the iSTFT, final samples -> the caller, and the next state slot.  Every move is a list of contiguous runs built on
// the host; one launch per list, one workgroup per run.  Pure copies: the bits are those of the kernels that made them.
#include "nhans_kernels.h"

namespace nhans {

__global__ void __launch_bounds__(256) online_copy_kernel(const OnlineCopy* __restrict__ runs) {
    const OnlineCopy r = runs[blockIdx.x];
    const int n = (int)r.n;
    for (int i = threadIdx.x; i < n; i += 256) r.dst[i] = r.src[i];
}

void launch_online_copy(const char* kernel, const OnlineCopy* runs_dev, int nruns, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, online_copy_kernel, dim3(nruns), dim3(256), 0, s, runs_dev);
}

}  // namespace nhans
