// What the transform kernels share (stft.hip, phase.hip): the feature math on the hardware transcendental units, the
// global-access form, the wavefront-private LDS exchange and the geometry of the 20 x 20 transpose.  Device code only.
#pragma once
#include "nhans_kernels.h"
#include "fft400.h"

namespace nhans {

constexpr int kFpw = 3;                 // iSTFT: transforms per wavefront
constexpr int kTRow = 21;               // padded transpose row (complex values)
constexpr int kTFrame = 20 * kTRow;     // 420 complex per frame
// ---- feature math on the hardware transcendental units.  Both kernels are VALU-bound once their loads
// are pipelined (PMC: 490 VALU wave-instructions per frame, two thirds of them libm's atan2f / logf /
// sincosf / expf with their full-range reductions); the ranges here are narrow and float32-level accuracy
// is all the path can use (phase 1.7e-7 rad, magnitudes ~2e-7 relative).
__device__ __forceinline__ float fast_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    // v_rcp_f32 takes no denormal input: it answers inf, and mn * inf is inf or NaN.  A bin whose larger component is below
    // the smallest normal number (a magnitude under 1.7e-38 beside the 1e-5 floor) counts as zero magnitude on the axis of
    // that component: 0, +-pi/2 or +-pi.  Normal inputs take the same instructions as before, bit for bit.
    const float r = mx >= 1.17549435e-38f ? mn * __builtin_amdgcn_rcpf(mx) : 0.f;     // atan2(0, 0) = 0 like libm
    const float t = r * r;
    // minimax fit of atan(r)/r in r^2 on [0, 1]: 1.7e-7 rad in float32 arithmetic
    float p = -0.004733146633952856f;
    p = fmaf(p, t, 0.024376805871725082f);
    p = fmaf(p, t, -0.0596301406621933f);
    p = fmaf(p, t, 0.09921535104513168f);
    p = fmaf(p, t, -0.140206977725029f);
    p = fmaf(p, t, 0.1996956467628479f);
    p = fmaf(p, t, -0.3333193361759186f);
    p = fmaf(p, t, 0.9999998807907104f);
    float a = p * r;
    a = ay > ax ? 1.57079632679489662f - a : a;
    a = x < 0.f ? 3.14159265358979324f - a : a;
    return copysignf(a, y);
}
__device__ __forceinline__ float fast_log(float v) {           // v >= 1e-5: v_log_f32 is log2, 1 ulp
    return __builtin_amdgcn_logf(v) * 0.69314718055994531f;
}
__device__ __forceinline__ float fast_exp(float x) {           // |x| < 60; the product x*log2(e) carried as hi + lo
    const float hi = x * 1.44269504088896341f;
    const float lo = fmaf(x, 1.44269504088896341f, -hi) + x * 1.925963033500e-8f;
    return __builtin_amdgcn_exp2f(hi) * fmaf(lo, 0.69314718055994531f, 1.0f);
}
__device__ __forceinline__ void fast_sincos(float a, float* sn, float* cs) {   // |a| <= pi: v_sin/v_cos take revolutions
    const float rev = a * 0.15915494309189535f;
    *sn = __builtin_amdgcn_sinf(rev);
    *cs = __builtin_amdgcn_cosf(rev);
}


// Global access as (wave-uniform 64-bit base) + (32-bit BYTE offset per lane): the form the scalar-base global
// instructions take directly; element indexing would make the compiler widen every offset to 64 bits first.
__device__ __forceinline__ float ldg32(const float* base, unsigned byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ void stg32(float* base, unsigned byte_off, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// A wavefront's transpose / spectrum area is private to it: its lanes exchange data through it with no
// workgroup barrier, only "my LDS traffic has completed" (lanes of a wave run in lockstep).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The ANALYSIS transform computes rows k1 = 0..10 of the transposed intermediate only (stft.hip: stft_features_kernel).
constexpr int kRows = 11;                    // rows k1 = 0..10 of the transposed intermediate
constexpr int kTReal = kRows * kTRow;        // 231 complex per frame

}  // namespace nhans
