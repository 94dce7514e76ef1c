// What the scoring kernels share (score.hip, mix.hip, stoi.hip, bsseval.hip, align.hip, quality.hip; level.hip takes the
// wavefront sum): the pieces their "a record's bits are a property of the clip pair" rests on, each written once.
#pragma once
#include "nhans_kernels.h"

namespace nhans {

// The run a workgroup belongs to: the last one whose first workgroup (member T0) is <= b.  The first workgroups ascend
// from 0 over the runs; a clip without a workgroup shares the value of the clip after it and is never the last, so it is
// never found.
template <typename Run, long long Run::*T0>
__device__ __forceinline__ int find_run(const Run* __restrict__ runs, int nruns, long long b) {
    int lo = 0, hi = nruns - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (runs[mid].*T0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the sum over a wavefront by the tree 32, ..., 1 in __dadd_rn: one fixed order whatever the batch (lane 0 holds the sum)
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off));
    return v;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// (host) whether a launch of ntiles workgroups over nruns runs goes ahead: nothing to do is no launch and no error, more
// workgroups than a grid's 2^31 - 1 a refusal noted under the launch's name
inline bool tiles_ok(const char* kernel, int nruns, long long ntiles) {
    if (nruns <= 0 || ntiles <= 0) return false;
    if (ntiles > 0x7fffffffLL) { note_refusal(kernel); return false; }
    return true;
}

}  // namespace nhans
