// Sample-rate conversion between 16 kHz and the rates capture devices deliver, and the peak normalisation of the file
// front end (include/nhans_hip.h: nhans_resample*, nhans_resampler_*, nhans_peak_normalise).
//
// The filter is the one scipy.signal.resample_poly(x, L, M) designs by default -- sinc times Kaiser(5) window of
// 2 * half + 1 taps, half = 10 max(L, M), unit sum, times L -- computed here in double so that a C caller needs no Python.
// Output m of a clip is
//     y[m] = sum_k h[m M + half - k L] x[k]  =  sum_{j < J} h[p + j L] x[q - j],   m M + half = q L + p,  0 <= p < L
// -- ONE chain of J fmaf in float32, j ascending, absent inputs as 0.0f (fir_chain below).  The offline call, the
// streaming push and both converters of a live session run ONE kernel body (resample_kernel) on run descriptors the
// host builds in one place (RateStage::add_runs, host_internal.h), so a stream's output cannot depend on how it was cut:
// a push only changes where an input sample is fetched from (the caller's new samples or the J carried ones), never the
// arithmetic on it.  The body is a template over a source (PCM int16 / float32, or the wet/dry mix of a live session
// formed while the span is staged) and a sink (float32 with the optional int16 grid and fixed peak, or scaled PCM);
// the six mono pairs in use are instantiated: int16 -> float, float32 -> float, and the fixed and the automatic mix ->
// int16 and -> float32 -- and, for live objects that take and return interleaved frames, the same six with the PCM side
// read from / stored into frames of several channels (InterleavedSource, InterleavedSink).  A full-band live object
// (nhans_fullband_*) runs its outgoing stage on eight more: the four mix pairs of either layout with the source
// wrapped in ResidualSource and the sink in HighbandSink, which add the input's own band above 8 kHz inside the launch;
// hold_kernel keeps the input samples that have no output yet.
#include "nhans_kernels.h"

#include <cmath>
#include <map>
#include <mutex>

namespace nhans {

// ---- design (host, double) ------------------------------------------------------------------------------------------
namespace {

double bessel_i0(double x) {
    // power series sum_k ((x/2)^k / k!)^2: every term positive, converges in < 30 terms for the x <= 5 used here
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

bool rate_supported(int r) {
    static const int ok[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000};
    for (int v : ok)
        if (v == r) return true;
    return false;
}

int gcd_int(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

ResampleFilter* design(int rate_in, int rate_out) {
    ResampleFilter* f = new ResampleFilter();
    f->rate_in = rate_in; f->rate_out = rate_out;
    const int g = gcd_int(rate_in, rate_out);
    f->L = rate_out / g; f->M = rate_in / g;
    if (f->L == 1 && f->M == 1) {       // a copy: fmaf(1, x, 0) = x
        f->half = 0; f->J = 1; f->h.assign(1, 1.0);
    } else {
        const int mx = std::max(f->L, f->M);
        f->half = 10 * mx;
        const int N = 2 * f->half + 1;
        const double cutoff = 1.0 / mx, alpha = 0.5 * (N - 1), beta = 5.0, pi = 3.14159265358979323846;
        const double i0b = bessel_i0(beta);
        f->h.resize(N);
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            const double m = n - alpha, a = pi * cutoff * m;
            const double sinc = m == 0.0 ? 1.0 : std::sin(a) / a;
            const double r = m / alpha;
            const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            f->h[n] = cutoff * sinc * w;
            sum += f->h[n];
        }
        for (int n = 0; n < N; ++n) f->h[n] = f->h[n] / sum * f->L;
        f->J = (N + f->L - 1) / f->L;
    }
    const size_t n = (size_t)f->L * f->J;
    f->tab.assign((n + 3) / 4 * 4, 0.f);
    for (int j = 0; j < f->J; ++j)
        for (int p = 0; p < f->L; ++p) {
            const size_t t = (size_t)p + (size_t)j * f->L;
            if (t < f->h.size()) f->tab[(size_t)j * f->L + p] = (float)f->h[t];
        }
    return f;
}

}  // namespace

namespace {

// the design of a pair, computed once per process
const ResampleFilter* filter_of(int rate_in, int rate_out) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, ResampleFilter*> cache;    // (lives as long as the process)
    std::lock_guard<std::mutex> lock(mu);
    ResampleFilter*& f = cache[{rate_in, rate_out}];
    if (!f) f = design(rate_in, rate_out);
    return f;
}

}  // namespace

const ResampleFilter* resample_filter(int rate_in, int rate_out) {
    if ((rate_in != 16000 && rate_out != 16000) || !rate_supported(rate_in) || !rate_supported(rate_out)) return nullptr;
    return filter_of(rate_in, rate_out);
}

const ResampleFilter* resample_filter_stoi() { return filter_of(16000, 10000); }

int64_t resample_out_count(const ResampleFilter& f, int64_t n) { return (n * f.L + f.M - 1) / f.M; }

// Output m is final once input q(m) = floor((m M + half) / L) exists: m M + half < N L.
int64_t resample_emitted(const ResampleFilter& f, int64_t n, bool ended) {
    const int64_t all = resample_out_count(f, n);
    if (ended) return all;
    const int64_t a = n * f.L - 1 - f.half;
    return std::min(all, a < 0 ? (int64_t)0 : a / f.M + 1);
}

size_t resample_run_lds_bytes(const ResampleFilter& f, int p0, int cnt) {
    const size_t span = cnt > 0 ? (size_t)((p0 + (int64_t)(cnt - 1) * f.M) / f.L + f.J) : 0;
    return (f.tab.size() + span) * sizeof(float);
}

// ---- kernels --------------------------------------------------------------------------------------------------------
namespace {

// The one accumulation every output of the library's rate conversion goes through: taps h[p + j L] at tab_p[j * L]
// (LDS), inputs x[q - j] at x_q[-j] (LDS), j ascending.
__device__ __forceinline__ float fir_chain(const float* tab_p, int L, const float* x_q, int J) {
    float acc = 0.f;
    for (int j = 0; j < J; ++j) acc = fmaf(tab_p[j * L], x_q[-j], acc);
    return acc;
}

// Sample rel of PCM at src as float32 (int16 -> float32 is exact) ...
template <typename T>
__device__ __forceinline__ float pcm_sample(const void* src, long long rel) {
    return (float)static_cast<const T*>(src)[rel];
}
// ... and of PCM frames of ch channels at src: the mean of the first `sum` channels of frame rel (InterleavedSource below)
template <typename T>
__device__ __forceinline__ float frame_sample(const void* src, long long rel, int ch, int sum) {
    const T* f = static_cast<const T*>(src) + rel * ch;
    double acc = 0.0;
    for (int c = 0; c < sum; ++c) acc += (double)f[c];
    return (float)(acc / (double)sum);
}

// Source policies: sample k0 + rel of the run's stream, 0 <= rel < n_new, as float32.
// PCM at src:
template <typename T>
struct PcmSource {
    static __device__ __forceinline__ float at(const ResampleRun& r, long long rel, float) { return pcm_sample<T>(r.src, rel); }
};
// PCM frames of r.src_ch channels at src, the sample being the mean of the first r.src_sum channels of its frame as
// channel_mean_kernel forms it: summed in double from 0.0, channel ascending, divided by double(r.src_sum), rounded to
// float32 once.  Summing ONE channel gives that channel's sample itself (0.0 + double(s)) / 1.0 -- exact for int16 and
// float32; -0.0f comes out as 0.0f, which no fmaf chain that starts at 0.0f can tell apart --, so a slot that owns one
// channel of a frame and a slot that is the frame's downmix are one policy.  The span that is staged, and therefore LDS,
// the lane -> output map and the carried samples, are those of a mono stream: after this function the stream is mono.
template <typename T>
struct InterleavedSource {
    static __device__ __forceinline__ float at(const ResampleRun& r, long long rel, float) {
        return frame_sample<T>(r.src, rel, r.src_ch, r.src_sum);
    }
};
// d + (m - d) * w in three separately rounded float32 operations (numpy's `den + (mix - den) * factor`).  The pragma is
// what keeps them apart: the _rn intrinsics are plain operators compiled under the translation unit's contraction mode,
// and the compiler fuses their product into the sum -- one rounding instead of two, a last-bit difference for every
// factor that is not a power of two.
__device__ __forceinline__ float mix_sample(float d, float m, float w) {
#pragma clang fp contract(off)
    const float r = m - d;
    const float p = r * w;
    return d + p;
}

// the combined stream c of a live session, stored nowhere: mix_sample of the push's two pieces, never contracted; with
// mix == nullptr (wet factor 0) c is den and mix is not read
struct MixSource {
    static __device__ __forceinline__ float at(const ResampleRun& r, long long rel, float wet) {
        const float d = static_cast<const float*>(r.src)[rel];
        if (!r.mix) return d;
        return mix_sample(d, r.mix[rel], wet);
    }
};
// the same with the hop's own factor from the push's gain table (level.hip wrote it, one launch earlier on the stream)
// where MixSource takes the scalar: hop (k0 + rel) / 160 of the stream, entry 0 of the table being hop r.hop0
struct AutoMixSource {
    static __device__ __forceinline__ float at(const ResampleRun& r, long long rel, float) {
        const float d = static_cast<const float*>(r.src)[rel];
        return mix_sample(d, r.mix[rel], r.wtab[(r.k0 + rel) / kHop - r.hop0]);
    }
};

// The full-band residual e = c - g * mix of a live session (include/nhans_hip.h: nhans_fullband_*), c what Mix gives:
// product and difference rounded separately, as mix_sample's.  mix is read whatever the wet factor is.  What the stage
// carries from push to push (hist / hist_out) is e, with the gain of the push that staged it.
template <typename Mix>
struct ResidualSource {
    static __device__ __forceinline__ float at(const ResampleRun& r, long long rel, float wet) {
#pragma clang fp contract(off)
        const float c = Mix::at(r, rel, wet);
        const float p = r.hb_gain * r.mix[rel];
        return c - p;
    }
};

// Sample n of a stream's own incoming signal x, for base <= n < n_end: from the slot's hold half below n_old, from the
// caller's PCM from there on, formed as the incoming stage's source forms it (fmt: int16 / float32; ch == 0: mono, else
// frames of ch channels, the first `sum` averaged).  The one reader of both the full-band sinks and hold_kernel.
__device__ __forceinline__ float stream_sample(const float* hold, long long base, long long n_old, const void* in, int fmt, int ch,
                                               int sum, long long n) {
    if (n < n_old) return n >= base && hold ? hold[n - base] : 0.f;
    const long long rel = n - n_old;
    if (ch == 0) return fmt == kResampleInt16 ? pcm_sample<int16_t>(in, rel) : pcm_sample<float>(in, rel);
    return fmt == kResampleInt16 ? frame_sample<int16_t>(in, rel, ch, sum) : frame_sample<float>(in, rel, ch, sum);
}

// Sink policies: what becomes of output i of the run, y = its chain.
// float32, optionally rounded to the int16 grid, then float32(double(v) / factor) when factor != 0 (the fixed peak):
struct FloatSink {
    static __device__ __forceinline__ void put(const ResampleRun& r, int i, float v, int quantise, double factor) {
        if (quantise) v = fminf(fmaxf(rintf(v), -32768.f), 32767.f);
        if (factor != 0.0) v = (float)((double)v / factor);
        static_cast<float*>(r.dst)[i] = v;
    }
};
// PCM: float32(double(y) * factor), then rounded and clamped for int16.  The int16 stores are plain 2-byte stores: a
// slot's destination is only 2-byte aligned, and the 64 lanes of a wave write 128 consecutive bytes.
template <typename T>
struct PcmSink {
    static __device__ __forceinline__ void put(const ResampleRun& r, int i, float y, int, double factor) {
        const float v = (float)((double)y * factor);
        if constexpr (sizeof(T) == 2) static_cast<int16_t*>(r.dst)[i] = (int16_t)fminf(fmaxf(rintf(v), -32768.f), 32767.f);
        else static_cast<float*>(r.dst)[i] = v;
    }
};
// The same value into frames of r.dst_ch channels: output i goes to the first r.dst_copies channels of frame i at dst (a
// slot that owns one channel writes 1, a downmix played on every channel writes them all).  Still plain 2-byte stores
// for int16: the lanes of a wave now write 2 bytes every 2 * dst_ch, and the copies of one lane are neighbours.
template <typename T>
struct InterleavedSink {
    static __device__ __forceinline__ void put(const ResampleRun& r, int i, float y, int, double factor) {
        const float v = (float)((double)y * factor);
        const int at = i * r.dst_ch;
        if constexpr (sizeof(T) == 2) {
            const int16_t q = (int16_t)fminf(fmaxf(rintf(v), -32768.f), 32767.f);
            for (int c = 0; c < r.dst_copies; ++c) static_cast<int16_t*>(r.dst)[at + c] = q;
        } else {
            for (int c = 0; c < r.dst_copies; ++c) static_cast<float*>(r.dst)[at + c] = v;
        }
    }
};

// The full-band sink: y = lo + g * u[n] for output n = hb_m0 + i of the stream, two separately rounded operations, then
// Inner's arithmetic and store.  u[n] = float32(double(x[n]) / hb_denom) -- FloatSink's division -- and 0 from the end
// of the stream's input on.
template <typename Inner>
struct HighbandSink {
    static __device__ __forceinline__ void put(const ResampleRun& r, int i, float lo, int quantise, double factor) {
#pragma clang fp contract(off)
        const long long n = r.hb_m0 + i;
        float u = 0.f;
        if (n < r.hb_n_end)
            u = (float)((double)stream_sample(r.hb_hold, r.hb_base, r.hb_n_old, r.hb_in, r.hb_fmt, r.hb_ch, r.hb_sum, n) / r.hb_denom);
        const float p = r.hb_gain * u;
        Inner::put(r, i, lo + p, quantise, factor);
    }
};

// sample k0 + rel of the run's stream: the source's where the push brought it, the carried one before that, else 0.0f
template <typename Src>
__device__ __forceinline__ float run_sample(const ResampleRun& r, long long rel, int J, float wet) {
    if (rel >= r.n_new) return 0.f;
    if (rel >= 0) return Src::at(r, rel, wet);
    const long long a = rel + J;
    if (a >= 0 && r.k0 + rel >= 0 && r.hist) return r.hist[a];
    return 0.f;
}

// One workgroup per run, one lane per output (4 rounds of 256 for a full run).  LDS: the phase table (phase-minor, so
// that for L = 1 every lane reads one address -- a broadcast --, for L = 2, 3, 6 the 64 lanes share that many addresses,
// and for the large L neighbouring lanes, whose phases differ by M mod L, land M mod L banks apart: conflict-free where
// that step is odd (44.1 -> 16 kHz: 121), 2-way and more where it is even (16 -> 44.1 kHz: 160 -- the price of one
// layout for every pair), then the input span of the run (<= 58.5 KB together, 88.2 kHz in).  Lane i reads x at stride
// M / L: 2-way bank conflicts for the even ratios (32 and 96 kHz in), none for 48 kHz in and for every upsampling pair.
// Src and Sink change only where a sample of the span comes from and what is stored; wet is the source's argument,
// quantise and factor are the sink's.
template <typename Src, typename Sink>
__global__ void __launch_bounds__(256) resample_kernel(const ResampleRun* __restrict__ runs, const float* __restrict__ tab,
                                                       int L, int M, int J, int tab4, int quantise, float wet, double factor) {
    extern __shared__ float4 rs_lds[];
    float* tl = reinterpret_cast<float*>(rs_lds);
    float* xs = tl + 4 * tab4;
    const ResampleRun r = runs[blockIdx.x];
    const int tid = threadIdx.x;
    for (int i = tid; i < tab4; i += 256) rs_lds[i] = reinterpret_cast<const float4*>(tab)[i];
    const int span = r.cnt > 0 ? (r.p0 + (r.cnt - 1) * M) / L + J : 0;
    const long long lo = r.qrel0 - (J - 1);
    for (int s = tid; s < span; s += 256) xs[s] = run_sample<Src>(r, lo + s, J, wet);
    __syncthreads();
    for (int i = tid; i < r.cnt; i += 256) {
        const int t = r.p0 + i * M;
        const int q = t / L, p = t - q * L;
        Sink::put(r, i, fir_chain(tl + p, L, xs + (J - 1) + q, J), quantise, factor);
    }
    if (r.hist_out)
        for (int t = tid; t < J; t += 256) r.hist_out[t] = run_sample<Src>(r, (long long)r.n_new - J + t, J, wet);
}

// One workgroup per run: x[e_new .. n_end) of a full-band slot into the half its next push reads (HoldRun).
__global__ void __launch_bounds__(256) hold_kernel(const HoldRun* __restrict__ runs) {
    const HoldRun r = runs[blockIdx.x];
    const long long n = r.n_end - r.e_new;
    for (long long t = threadIdx.x; t < n; t += 256)
        r.out[t] = stream_sample(r.old, r.base, r.n_old, r.in, r.fmt, r.ch, r.sum, r.e_new + t);
}

__device__ __forceinline__ float block_max(float m) {
    __shared__ float part[4];
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// wrap: |-32768| counts as -32768, what np.abs of an int16 array gives (the reference's normalise on a mono file)
__global__ void __launch_bounds__(256) peak_partial_kernel(const float* __restrict__ x, const NormBlock* __restrict__ blocks,
                                                           int wrap, float* __restrict__ partial) {
    const NormBlock b = blocks[blockIdx.x];
    const float* p = x + b.off;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < b.n; i += 256) {
        const float v = p[i];
        m = fmaxf(m, (wrap && v == -32768.f) ? v : fabsf(v));
    }
    m = block_max(m);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ void __launch_bounds__(256) peak_normalise_kernel(const float* x, const NormBlock* __restrict__ blocks,
                                                             const float* __restrict__ partial, float* out) {
    const NormBlock b = blocks[blockIdx.x];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < b.pbn; i += 256) m = fmaxf(m, partial[b.pb0 + i]);
    m = block_max(m);
    const double den = (double)m + 0.000001;
    for (int i = threadIdx.x; i < b.n; i += 256) out[b.off + i] = (float)((double)x[b.off + i] / den);
}

// out[i] = float32(mean over the channels of in[c * n + i], summed in double): the host converter's x.mean(axis = 1)
__global__ void __launch_bounds__(256) channel_mean_kernel(const float* in, int nchan, long long n, float* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int c = 0; c < nchan; ++c) acc += (double)in[(long long)c * n + i];
    out[i] = (float)(acc / (double)nchan);
}

}  // namespace

void launch_channel_mean(const float* in, int nchan, int64_t n, float* out, hipStream_t s) {
    if (n <= 0) return;
    NHANS_LAUNCH("channel_mean", channel_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, nchan, (long long)n, out);
}

void launch_resample(const char* kernel, const ResampleRun* runs_dev, int nruns, const float* tab_dev, const ResampleFilter& f,
                     bool from_mix, bool auto_wet, bool interleaved, int pcm_format, int quantise, float wet, double factor,
                     size_t lds_bytes, hipStream_t s, bool highband) {
    if (nruns <= 0) return;
    if (lds_bytes > (size_t)64 << 10) { note_refusal(kernel); return; }
    const int tab4 = (int)(f.tab.size() / 4);
    const bool i16 = pcm_format == kResampleInt16;
    auto* mono = !from_mix ? (i16 ? resample_kernel<PcmSource<int16_t>, FloatSink> : resample_kernel<PcmSource<float>, FloatSink>)
                 : !auto_wet ? (i16 ? resample_kernel<MixSource, PcmSink<int16_t>> : resample_kernel<MixSource, PcmSink<float>>)
                             : (i16 ? resample_kernel<AutoMixSource, PcmSink<int16_t>> : resample_kernel<AutoMixSource, PcmSink<float>>);
    auto* fn = mono;
    if (interleaved)
        fn = !from_mix ? (i16 ? resample_kernel<InterleavedSource<int16_t>, FloatSink> : resample_kernel<InterleavedSource<float>, FloatSink>)
             : !auto_wet ? (i16 ? resample_kernel<MixSource, InterleavedSink<int16_t>> : resample_kernel<MixSource, InterleavedSink<float>>)
                         : (i16 ? resample_kernel<AutoMixSource, InterleavedSink<int16_t>>
                                : resample_kernel<AutoMixSource, InterleavedSink<float>>);
    if (highband && from_mix) {
        using Fixed = ResidualSource<MixSource>;
        using Auto = ResidualSource<AutoMixSource>;
        if (!interleaved)
            fn = !auto_wet ? (i16 ? resample_kernel<Fixed, HighbandSink<PcmSink<int16_t>>> : resample_kernel<Fixed, HighbandSink<PcmSink<float>>>)
                           : (i16 ? resample_kernel<Auto, HighbandSink<PcmSink<int16_t>>> : resample_kernel<Auto, HighbandSink<PcmSink<float>>>);
        else
            fn = !auto_wet ? (i16 ? resample_kernel<Fixed, HighbandSink<InterleavedSink<int16_t>>>
                                  : resample_kernel<Fixed, HighbandSink<InterleavedSink<float>>>)
                           : (i16 ? resample_kernel<Auto, HighbandSink<InterleavedSink<int16_t>>>
                                  : resample_kernel<Auto, HighbandSink<InterleavedSink<float>>>);
    }
    NHANS_LAUNCH(kernel, fn, dim3(nruns), dim3(256), lds_bytes, s, runs_dev, tab_dev, f.L, f.M, f.J, tab4, quantise, wet, factor);
}

void launch_hold(const char* kernel, const HoldRun* runs_dev, int nruns, hipStream_t s) {
    if (nruns <= 0) return;
    NHANS_LAUNCH(kernel, hold_kernel, dim3(nruns), dim3(256), 0, s, runs_dev);
}

void launch_peak_partial(const float* x, const NormBlock* blocks_dev, int nblocks, int wrap, float* partial, hipStream_t s) {
    if (nblocks <= 0) return;
    NHANS_LAUNCH("peak_partial", peak_partial_kernel, dim3(nblocks), dim3(256), 0, s, x, blocks_dev, wrap, partial);
}

void launch_peak_normalise(const float* x, const NormBlock* blocks_dev, int nblocks, const float* partial, float* out,
                           hipStream_t s) {
    if (nblocks <= 0) return;
    NHANS_LAUNCH("peak_normalise", peak_normalise_kernel, dim3(nblocks), dim3(256), 0, s, x, blocks_dev, partial, out);
}

}  // namespace nhans
