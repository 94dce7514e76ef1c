// Internal declarations shared by the HIP translation units of libnhans_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <utility>
#include <vector>

namespace nhans {

constexpr int kWin = 400, kHop = 160, kBins = 201, kMixWin = 35, kCtxFrames = 200, kEmb = 512;
constexpr int kCenter = kMixWin / 2;
// frame windows per pass of the stack: frames x 35 x 201 x 64 elements < 2^31 (32-bit element offsets in the conv kernels)
constexpr int64_t kMaxFramesPerChunk = ((int64_t)1 << 31) / ((int64_t)kMixWin * kBins * 64);

// Developer tooling (cycle stamps, timing ablations that compute WRONG results, kernel-choice
// switches read from the environment) exists only in a `make DEV=1` build (-DNHANS_DEV); the
// default library contains none of it.
#ifdef NHANS_DEV
constexpr bool kDev = true;
int dev_ablate();          // getenv("NHANS_ABLATE"), read once
#else
constexpr bool kDev = false;
constexpr int dev_ablate() { return 0; }
#endif

// ---------------------------------------------------------------------------------------------
// Launch-error channel (launch_status.hip).  Every kernel of the library is launched through NHANS_LAUNCH, which takes
// the launch's OWN return code (hipLaunchKernel) -- not the runtime's sticky per-thread "last error", which an earlier
// HIP call of the application may have left set and which is neither blamed on this library nor consumed on the
// application's behalf --, and set_max_dynamic_lds() runs before a launch that needs more than 64 KB of LDS; the first
// failure of the calling thread is kept until the C-ABI entry point collects it with take_launch_error() and returns
// NHANS_EHIP.  Nothing is launched silently wrong.
void note_launch(const char* kernel, hipError_t launch_rc);
bool launch_error_pending();                // a launch of this thread's current call has failed or been refused (not cleared)
void note_refusal(const char* what);        // a launch the library itself refuses: reported as hipErrorInvalidValue, no HIP state touched
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute: `done_mask` (one static per
// kernel instantiation) has one bit per device id.
void set_max_dynamic_lds(const void* fn, size_t bytes, unsigned long long* done_mask, const char* kernel);
hipError_t take_launch_error(const char** kernel);
template <typename... P, size_t... I>
inline hipError_t launch_packed(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, std::tuple<std::decay_t<P>...>& params,
                                std::index_sequence<I...>) {
    void* ptrs[] = {static_cast<void*>(&std::get<I>(params))...};
    return hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, s);
}
template <typename... P, typename... A>
inline void launch_checked(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
    std::tuple<std::decay_t<P>...> params(std::forward<A>(args)...);        // converted to the kernel's parameter types
    note_launch(name, launch_packed<P...>(kernel, grid, block, lds, s, params, std::index_sequence_for<P...>{}));
}
#define NHANS_LAUNCH(NAME, KERNEL, GRID, BLOCK, LDS, STREAM, ...)                                  \
    ::nhans::launch_checked(NAME, KERNEL, GRID, BLOCK, LDS, STREAM, __VA_ARGS__)

// bit set in *sat by the split-f16 writers when an activation does not fit f16 (|v| >= 65504 or NaN)
constexpr int kSatActivation = 1;
// conv_wino.hip re-splits V = BT d into f16: for the non-negative (post-ReLU) tensors it reads, |V| <= 8.5 max d -- the
// largest one-signed coefficient sum of a BT row of F(5,4) -- and the f16 conversion saturates SILENTLY, so the launch
// that writes such a tensor raises the flag at 65504 / 8.5 = 7,706 already (7,168 leaves room for the f32 rounding).
constexpr float kSatLimitF16 = 65504.f, kSatLimitWinoInput = 7168.f;

// Division by a runtime constant for numerators < 2^31 (Granlund-Montgomery round-up form).
struct FastDiv {
    uint32_t d, mul, sh;
};
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    f.mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
    f.sh = l;
    return f;
}
__device__ __forceinline__ uint32_t fd_div(uint32_t n, const FastDiv& f) {
    return (__umulhi(f.mul, n) + n) >> f.sh;
}

// A batch of 1-channel "images" that are SLIDING WINDOWS of one [rows, W] tensor: image b's row h is tensor row
// row0 + b + h when 0 <= t[b] + h - pad < T[b] (t: the frame's position in its clip, T: the clip's length), and a row of
// 0.0 otherwise -- strided_crop of SN/apply.py:170-186,378 (35-row windows of the log-magnitude spectrogram, zero rows
// -- not the silence floor -- outside the clip) without ever materialising [T, 35, 201].
// t == nullptr: plain images [B, H, W].
// rb != nullptr (online enhancement, host_online.hip): image b's row h is tensor row rb[b] + h instead -- the frames of one
// launch then need not be consecutive rows of one tensor (each online stream brings its own history and look-ahead rows)
struct WinRows {
    const int* t;
    const int* T;
    int row0, pad;      // (row0 may be negative: host_net.hip counts rows from the launch's first frame, row0 = -pad)
    const int* rb;      // nullable: per-image first row (row0 is then unused)
};
constexpr int kNoRow = -2147483647 - 1;      // "this row is a zero row" where an element index is stored (conv_epilogue.h)
__device__ __forceinline__ bool win_row_ok(const WinRows& w, int b, int h) {
    return (unsigned)(w.t[b] + h - w.pad) < (unsigned)w.T[b];
}
__device__ __forceinline__ int win_row(const WinRows& w, int b, int h) {
    return (w.rb ? w.rb[b] : w.row0 + b) + h;
}

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution on the f32 matrix cores (conv_igemm.hip).
//   out[m, n] = epilogue( sum_seg sum_{kh,kw,c} src_seg[b, ho*sh+kh-pt, wo*sw+kw-pl, c] * W_seg[kh,kw,c,n] )
// with m = (b*Ho + ho)*Wo + wo.  Up to two K segments: the kxk taps of the block's main conv and
// (for blocks that change channel count) the 1x1 strided `_transform` conv folded in as extra K.
struct ConvSeg {
    const float* src;   // NHWC [B, H, W, C]
    const float* wpk;   // packed weights [chunk][N/32][4][64][4] (see fold.py: pack_igemm)
    int H, W, C;
    int KH, KW, sh, sw, pt, pl;
    int nchunks;        // KH*KW*C/32
    // Row-class launches (host_net.hip: row_classes): this launch applies only the filter rows kh0 .. kh0 + KH - 1 of a
    // filter of KHfull rows -- wpk is still the whole filter's array, packed (32-channel chunk, kh, kw), and pt is the
    // class's own, pt - kh0 - oh0*sh (may be negative).  An ordinary launch has kh0 = 0, KHfull = KH.  Only the halo
    // kernel and its pointwise mode read these.
    int kh0, KHfull;
};

struct ConvArgs {
    ConvSeg seg[2];
    int nseg;
    int Ho, Wo;
    int M;              // B*Ho*Wo
    // Output view (conv_epilogue.h): the launch's Ho rows are rows oh0 .. oh0 + Ho - 1 of an output image of Ho_full rows
    // -- position table, stored pixel and one-channel residual take row oh0 + ho.  Ordinary launch: oh0 = 0, Ho_full = Ho.
    int oh0, Ho_full;
    int N;              // padded output channels (multiple of the N tile)
    int Nreal;          // stored channels
    int ldo;            // out row stride
    float* out;
    // epilogue: v = acc + cb[clip(b)*cb_stride + n] + tf[(ho*Wo+wo)*N + n]
    //           aux[m*aux_ld+n] = v (optional)
    //           v += idw[n]*id[m*id_ld+n]                       (id_mode 1: same-shape tensor)
    //           v += idw[n]*ids[(b*idH + ho*idsh)*idW + wo*idsw] (id_mode 2: 1-channel image)
    //           out = relu ? max(v,0) : v
    const float* cb;
    int cb_stride;
    const int* img_clip;   // nullable -> clip 0
    const float* tf;       // nullable: time+frequency position table [Ho*Wo, N]
    const float* tt;       // the same table's two terms on their own, [Ho, N] and [Wo, N] (conv_wino.hip reads these:
    const float* ff;       // 60 KB instead of 1.8 MB per layer); nullable together
    int id_mode;
    const float* id;
    int id_ld;
    const float* idw;
    int idH, idW, idsh, idsw;
    WinRows id_win;        // id_mode 2: the image is a sliding window of `id` (idH is then unused)
    int relu;
    float* aux;
    int aux_ld;
    const float* zero;     // one readable 0.0f (stands in for absent tables / residuals)
    int prec;              // 0: f32 MFMA on f32 NHWC; 1: split-f16 x3 MFMA on split NHWC inputs
    int out_split;         // write `out` as split NHWC (ldo = N words per pixel) instead of f32
    int id_split;          // id_mode 1 tensor is split NHWC
    int in_f32;            // prec 1 only: seg[0].src is f32 NHWC (scaled like a split tensor) -- a tensor that only Winograd
                           // launches read (conv_wino.hip, the one kernel that takes it)
    const float* ws;       // prec 1: per-channel power-of-two that undoes the weight pre-scaling
    // Split-f16 tensors are STORED times a per-tensor power of two 2^-e (host_internal.h: activation exponents), so that
    // what a trained or an odd model produces stays inside the f16 range.  The epilogue computes in the unscaled
    // domain, bit for bit what it computes with e = 0: ws is multiplied by in_scale = 2^e(input), idw by id_scale =
    // 2^e(residual), and the result by out_scale = 2^-e(output) on its way to memory.  All three are 1 for f32 tensors.
    float in_scale, id_scale, out_scale;
    // the flag is raised by a stored |value| >= sat_limit: 65504 (the f16 range), or kSatLimitWinoInput for a tensor the
    // next launch reads in its Winograd form
    float sat_limit;
    int* sat;              // prec 1: device flag word, kSatActivation is OR-ed in when a stored activation saturates
    int variant;           // 0: 128-pixel / 4-wave register-staged kernel, 1: 256-pixel / 8-wave LDS-DMA kernel,
                           // 2: LDS-DMA kernels with producer / consumer waves and halo reuse across the KW taps
    int epi8;              // split-NHWC outputs: 8 channels per thread in the epilogue sweep (16-byte pieces), default;
                           // 0 = the 4-channel sweep (A/B and parity cross-check; same bits)
    int ilv;               // halo kernel: operand reads between the MFMAs, front-loaded in each half (default 1); 2 = spread
                           // evenly over the half; 0 = read block then MFMA block (the round-1 order) -- A/B knob, same bits
    int halo64_tile512;    // halo kernel, 64-channel convs: 512-pixel tiles (set by the launcher)
    long long* dbg;        // NHANS_DEV builds only: 4 s_memtime stamps per workgroup [start, loop, epilogue, end]
    FastDiv fdHoWo, fdWo;
    FastDiv fdWP;          // Wo + KW - 1 (filled in by launch_conv_igemm_halo)
    // split-K scratch (conv_igemm_dma.hip; null = never split): partial accumulator tiles and one
    // zero-initialised ticket counter per output tile
    float* kscratch;
    size_t kscratch_bytes;
    int* kcounter;
    int kcounter_n;
    int kgroup;            // caller: -1 = this layer may use grouped summation / split-K, 0 = never;
                           // the launcher turns -1 into the chunks per group
    // 1-D Winograd along W (conv_wino.hip).  Caller: wino_u / wino_ws (null = this conv has no Winograd form) and
    // wino on/off; the launcher fills in the rest: outputs per tile, tile-pixel block (rows x tiles, <= 64), blocks
    // per frame, tiles per image row
    const float* wino_u;
    const float* wino_ws;
    int wino;
    int wino_m, wino_tr, wino_tj, wino_nrb, wino_ncb, wino_ntile;
    FastDiv wino_fd_bpf, wino_fd_nnb, wino_fd_ncb;   // blocks per frame, channel blocks, column blocks (block decode)
};

// returns algorithmic FLOPs of the launch (2*M*K*Nreal); *kernel (optional) names the variant that ran
// *mfma_flops (optional): FLOPs the matrix cores actually execute for it -- 3 products per MAC in split-f16 mode,
// and 8*KH instead of m*KW*KH products per tile for a conv that runs in its Winograd form
double launch_conv_igemm(const ConvArgs& a, hipStream_t s, const char** kernel = nullptr, double* mfma_flops = nullptr);
double conv_wino_mfma_flops(const ConvArgs& a);                 // conv_wino.hip
void launch_conv_igemm_dma(const ConvArgs& a, hipStream_t s);   // conv_igemm_dma.hip
size_t conv_splitk_scratch_bytes(const ConvArgs& a);            // conv_igemm_dma.hip: scratch its split-K form would need (0: no split)
bool conv_wino_eligible(const ConvArgs& a);                     // conv_wino.hip
void launch_conv_wino(const ConvArgs& a, hipStream_t s);
bool conv_igemm_halo_eligible(const ConvArgs& a);               // conv_igemm_halo.hip
void launch_conv_igemm_halo(const ConvArgs& a, hipStream_t s);
bool conv_igemm_halo_pw_eligible(const ConvArgs& a);            // the same pipeline without halo reuse (strided / VALID convs)
void launch_conv_igemm_halo_pw(const ConvArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// The stand-alone 1x1 strided `_transform` conv of resblock2_1 as a stream (conv_1x1_stream.hip): 64 split-NHWC channels in,
// 128 f32 channels out, out = (x W) * ws * in_scale -- the arithmetic of conv_igemm_dma.hip for that launch, bit for bit
struct Stream1x1Args {
    const float* src;      // split NHWC [B, H, W, 64]
    const float* wpk;      // fold.py pack_igemm_h3 of the [64, 128] matrix
    const float* ws;       // [128] per-channel power of two that undoes the weight pre-scaling
    float in_scale;
    float* out;            // f32 [M, 128]
    int H, W, sh, sw, M;
    FastDiv fdHoWo, fdWo;
};
bool conv_1x1_stream_eligible(const ConvArgs& t);
void launch_conv_1x1_stream(const ConvArgs& t, hipStream_t s);

// Small kernels (aux_kernels.hip)
struct DirectArgs {     // convolution of a 1-channel image into 64 channels, same epilogue terms
    const float* src;   // [B, H, W] -- or, win.t != nullptr, the [rows, W] tensor the images are sliding windows of
    WinRows win;
    const float* w;     // [KH*KW][64], BN scale folded in
    int H, W, KH, KW, sh, sw, pt, pl, Ho, Wo;
    int M;              // B*Ho*Wo
    float* out;         // [M, 64]
    const float* cb;
    int cb_stride;
    const int* img_clip;
    const float* tf;    // [Ho*Wo,64] nullable
    const float* tt;    // its two terms [Ho,64], [Wo,64]: used instead of tf when present (v = (acc + cb + tt) + ff)
    const float* ff;
    int relu;
    int out_split;      // write split NHWC (hi/lo f16) instead of f32
    float out_scale;    // as ConvArgs::out_scale
    float sat_limit;    // as ConvArgs::sat_limit
    int* sat;           // as ConvArgs::sat
    FastDiv fdHoWo, fdWo;
};
void launch_direct_conv64(const DirectArgs& a, hipStream_t s);
// split NHWC [M, C] -> f32 [M, C], times `scale`
void launch_unsplit(const float* src, int64_t M, int C, float scale, float* dst, hipStream_t s);
void launch_scale_copy(const float* src, size_t n, float scale, float* dst, hipStream_t s);   // dst = src * scale (an f32-stored tensor out of its exponent)
// *slot = max(*slot, scale * max|x|) over a tensor of `nwords` 32-bit words (f32 values, or pairs of f16 halfs of a
// split-NHWC tensor: the hi halfs dominate); *slot holds the bits of a non-negative float.  Calibration only.
void launch_absmax(const float* x, size_t nwords, int split, float scale, unsigned* slot, hipStream_t s);

// frame index: for global frame g -> clip, t within clip, T of clip as frame g sees it: min(len, t + lookahead + 1) --
// the window rows from there on read as 0.0 (WinRows).  lookahead = 17 (half the window): T = len for every frame.
void launch_frame_index(const int64_t* frame_offsets_dev, int nclips, int64_t total, int lookahead, int* f_clip,
                        int* f_t, int* f_T, hipStream_t s);
// mean over HW positions, times `scale`: x [B, HW, C] -> out [B, C]
void launch_avgpool(const float* x, int B, int HW, int C, int split, float scale, float* out, hipStream_t s);
// cb[clip, n] = base[n] + sum_k ea[clip,k]*Wc[k, n] + sum_k eb[clip,k]*Wc[512+k, n]
void launch_cond(const float* ea, const float* eb, int nclips, const float* Wc, const float* base,
                 int ncols, float* cb, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Online enhancement (online.hip): the state, gather and commit moves of nhans_online_push are lists of contiguous float
// runs, one workgroup per run (the host splits runs longer than kOnlineCopyMax)
struct OnlineCopy {
    const float* src;
    float* dst;
    long long n;        // floats, <= kOnlineCopyMax
};
constexpr int kOnlineCopyMax = 8192;
void launch_online_copy(const char* kernel, const OnlineCopy* runs_dev, int nruns, hipStream_t s);
// Conditioning captured from a slot's own stream (include/nhans_hip.h: nhans_capture_*): per slot a ring of the last
// kCaptureSamples 16 kHz samples, sample k of the stream at position k mod kCaptureSamples; one entry = one context clip
struct CaptureEntry {
    const float* ring;  // the slot's ring, kCaptureSamples floats, every one of them valid
    float* clip;        // kCaptureSamples floats out, oldest sample first
    int start;          // ring position of the oldest sample: N mod kCaptureSamples
    int normalise;      // != 0: through the arithmetic of nhans_peak_normalise (flags 0)
};
constexpr int kCaptureSamples = (kCtxFrames - 1) * kHop + kWin;     // 32,240: the 200 context frames
constexpr int kCaptureThreads = 1024;
void launch_capture_clip(const CaptureEntry* entries_dev, int n, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// STFT / iSTFT (stft.hip)
struct ClipTable {      // device arrays, one entry per clip
    const int64_t* sample_off;   // [nclips+1] offsets into the wav buffer
    const int64_t* frame_off;    // [nclips+1] offsets into [T_total,201] tensors
    const int64_t* out_off;      // [nclips+1] (iSTFT) offsets into the output wav buffer
};
// grid = one block per (clip, run of kStftFramesPerBlock frames); block_clip/block_f0 enumerate them
void launch_stft(const float* wav, ClipTable t, const int* block_clip, const int* block_f0, int nblocks,
                 const float* tw400 /*400 cplx*/, const float* window /*400*/, float* logmag,
                 float* phase, hipStream_t s);
void launch_istft(const float* logmag, const float* phase, ClipTable t, const int* block_clip,
                  const int* block_h0, int nblocks, const float* tw400, const float* wsyn /*400*/,
                  float* wav_out, hipStream_t s);
constexpr int kStftFramesPerBlock = 23;   // frames per run: 460 pass-1 tasks (256 + 204) and 253 pass-2 tasks on 256 lanes
constexpr int64_t kMaxFramesPerClip = 5000000;   // 13.9 h: the STFT / iSTFT kernels address a clip with 32-bit byte offsets
constexpr int kIstftHopsPerBlock = 22;    // output hops per block; needs 24 frames

// ---------------------------------------------------------------------------------------------
// Phase refinement (phase.hip; include/nhans_hip.h: nhans_phase_*).  Complex planes are [frames, 201] pairs of float32
// (re, im).  One projection launch: d = P(A, t) per clip of frame_off_dev, workgroups walking the (clip, first frame) runs
// of kPhaseRun frames in block_clip / block_f0 -- 24 inverse transforms (the run and two halo frames either side), the
// span's overlap-add in LDS, kPhaseRun forward transforms.  d_prev (nullable): t_out = d + alpha (d - d_prev), else
// t_out = d; d_out may be d_prev itself (an element is read and written by one lane); d_out, t_out and num (nullable) are
// written for the frames of the clip only.  num[frame] = sum_k (|d| - A)^2 in double, bins ascending.
constexpr int kPhaseRun = 20;
constexpr int kPhaseMaxIters = 256;
void launch_phase_project(const float* A, const float* t_in, const int64_t* frame_off_dev, const int* block_clip, const int* block_f0,
                          int nblocks, const float* tw400, const float* window, const float* wsyn, const float* d_prev, float alpha,
                          float* d_out, float* t_out, double* num, hipStream_t s);
// A = exp(logmag) and den[frame] = sum_k A^2 (double, bins ascending); phase (nullable, with t0): t0 = cos + i sin
void launch_phase_prepare(const float* logmag, const float* phase, int64_t nframes, float* A, float* t0, double* den, hipStream_t s);
// phase_out = angle(t), n elements
void launch_phase_angle(const float* t, int64_t n, float* phase_out, hipStream_t s);
// inc_out[clip * stride + col] = sum num / sum den over the clip's frames: lane l of 64 sums frames l, l + 64, ... ascending,
// the 64 sums by wave_sum (score_common.h)
void launch_phase_inc(const double* num, const double* den, const int64_t* frame_off_dev, int nclips, double* inc_out, int stride, int col,
                      hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Mask-driven MVDR beamforming (mvdr.hip; include/nhans_hip.h: nhans_mvdr_*).  X: complex rows, channel c of clip i at row
// C foff[i] + c T_i; mask, gain and the output rows: [F, 201] at foff; phi: complex double [nclips][2][C][C][201] (Phi_s,
// Phi_n); w: complex double [nclips][201][C]; rec: kMvdrFields doubles per clip.
constexpr int kMvdrMaxChannels = 8, kMvdrFields = 6, kMvdrLogGain = 1;
constexpr int kMvdrRun = 32;            // frames per workgroup of the filter
// the channel-clips of t (nclips * C of them) -> X and, where asked, the analysis rows of every channel-clip
void launch_mvdr_spectra(const float* wav, ClipTable t, const int* block_clip, const int* block_f0, int nblocks, const float* tw400,
                         const float* window, float* X, float* logmag, float* phase, hipStream_t s);
// the covariances into phi and each bin's sum |X_ref|^2 into eref [nclips][201]
void launch_mvdr_cov(const float* X, const float* mask, const int64_t* frame_off_dev, int nclips, int C, int ref, int flags, double* phi,
                     double* eref, hipStream_t s);
// phi -> w and (nullable) rec: frames, channels, ref, fallback_bins, energy_ref, NaN
void launch_mvdr_solve(const double* phi, const double* eref, const int64_t* frame_off_dev, int nclips, int C, int ref, double loading,
                       double* w_out, double* rec_out, hipStream_t s);
// the rows of y = w^H x (+ gain, nullable) over the (clip, first frame) runs of kMvdrRun frames; y (nullable): the complex
// float32 values themselves, [F, 201]; eframe (nullable): a frame's sum |y|^2
void launch_mvdr_apply(const float* X, const double* w, const float* gain, const int64_t* frame_off_dev, const int* block_clip,
                       const int* block_f0, int nblocks, int C, float* logmag, float* phase, float* y, double* eframe, hipStream_t s);
// rec[clip][5] = the sum of the clip's eframe: lane l of 64 sums frames l, l + 64, ... ascending, the 64 sums by wave_sum
void launch_mvdr_energy(const double* eframe, const int64_t* frame_off_dev, int nclips, double* rec, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Sample-rate conversion and the file front end (resample.hip; include/nhans_hip.h: nhans_resample*)
// The filter of scipy.signal.resample_poly(x, L, M), designed on the host in double.  tab = the taps rounded to float32,
// phase-minor: tab[j * L + p] = h[p + j * L] (0 beyond the last tap), padded to a multiple of 4 floats.
struct ResampleFilter {
    int rate_in = 0, rate_out = 0, L = 1, M = 1, half = 0, J = 1;
    std::vector<double> h;      // 2 * half + 1 taps
    std::vector<float> tab;     // L * J floats, padded
};
// nullptr for a pair that is not supported; the design of a pair is computed once per process (thread-safe)
const ResampleFilter* resample_filter(int rate_in, int rate_out);
// 16000 -> 10000 Hz (L = 5, M = 8, half = 80): the same design, for nhans_stoi_resample only -- not a pair of the public list
const ResampleFilter* resample_filter_stoi();
int64_t resample_out_count(const ResampleFilter& f, int64_t n);                 // ceil(n L / M)
int64_t resample_emitted(const ResampleFilter& f, int64_t n, bool ended);      // the streaming output contract

// One workgroup: outputs [m0, m0 + cnt) of one clip or stream, m0 * M + half = q0 * L + p0.  The input is the stream's
// samples from absolute index k0 on (n_new of them) preceded by `hist`, the J samples before k0 as float32 (entries of
// negative absolute index are never read); everything else reads as 0.0f.  The new samples are either PCM at src (int16
// or float32) or, for the outgoing stage of a live PCM session, stored nowhere: sample k0 + rel is
// c = den[rel] + (mix[rel] - den[rel]) * wet with den at src, formed while the span is staged (mix == nullptr: c = den,
// the wet factor is 0).  `hist` / `hist_out` carry what the source gives: x, or c.
struct ResampleRun {
    const void* src;
    const float* mix;       // the mix source only, nullable; the PCM source ignores it
    const float* hist;      // nullable: nothing before k0
    void* dst;              // float32 from PCM; int16 or float32 elements, by the launch's format, from the mix
    float* hist_out;        // non-null: this workgroup also writes the J samples before k0 + n_new (the stream's next history)
    long long k0;
    long long qrel0;        // q0 - k0
    int p0, n_new, cnt;
    // the automatic mix source only (level.hip), left zero by the run builder: the push's per-hop wet factors, entry 0
    // that of hop `hop0` of the stream -- sample k0 + rel takes wtab[(k0 + rel) / 160 - hop0] where the fixed mix takes wet
    const float* wtab;
    long long hop0;
    // the interleaved PCM source and sink only (live objects that take and return frames of several channels), left zero
    // by the run builder: src holds frames of src_ch channels and sample k0 + rel is the mean of the first src_sum of
    // frame rel, summed in double, channel ascending (1: that channel itself); dst holds frames of dst_ch channels and
    // output i is stored into the first dst_copies of frame i.  A slot that owns channel c of its frames has src / dst
    // point at that channel of the first frame.
    int src_ch, src_sum, dst_ch, dst_copies;
    // the full-band source and sink only (include/nhans_hip.h: nhans_fullband_*), left zero by the run builder.  The
    // source gives e = c - hb_gain * mix[rel] where the mix sources give c (mix is then never null).  Output i of the run
    // is output hb_m0 + i = n of the stream, and the sink stores lo + hb_gain * u[n] where the plain sinks store lo:
    // u[n] = float32(double(x[n]) / hb_denom), x[n] the stream's own incoming sample n -- hb_hold[n - hb_base] for
    // hb_base <= n < hb_n_old (the slot's hold half), the caller's PCM at hb_in for hb_n_old <= n < hb_n_end (sample
    // n - hb_n_old of it: hb_fmt int16 / float32 elements, hb_ch == 0 mono, else frames of hb_ch channels of which the
    // first hb_sum are averaged as the interleaved source does) -- and u[n] = 0 from hb_n_end on.
    const float* hb_hold;
    const void* hb_in;
    long long hb_base, hb_n_old, hb_n_end, hb_m0;
    double hb_denom;
    float hb_gain;
    int hb_fmt, hb_ch, hb_sum;
};
constexpr int kResampleRun = 1024;      // outputs per workgroup at most
constexpr int kResampleInt16 = 0, kResampleFloat32 = 1;
size_t resample_run_lds_bytes(const ResampleFilter& f, int p0, int cnt);
// from_mix false: PCM of pcm_format -> float32, rounded to the int16 grid with `quantise`, then float32(double(y) / factor)
// when factor != 0 (the fixed-peak normalisation of a live stream).  from_mix true: the wet/dry mix -> PCM of pcm_format,
// float32(double(y) * factor) before the rounding.  A run table that needs more than 64 KB of LDS is refused.
// auto_wet (from_mix only): the wet factor of a sample is its hop's entry of the run's gain table, not `wet`.
// interleaved: the PCM side -- the source from PCM, the sink from the mix -- is frames of several channels, laid out by the
// runs' src_ch / src_sum or dst_ch / dst_copies.
// highband (from_mix only): the full-band source and sink, on the runs' hb_ fields.
void launch_resample(const char* kernel, const ResampleRun* runs_dev, int nruns, const float* tab_dev, const ResampleFilter& f,
                     bool from_mix, bool auto_wet, bool interleaved, int pcm_format, int quantise, float wet, double factor,
                     size_t lds_bytes, hipStream_t s, bool highband = false);

// The hold of a full-band live slot: samples [e_new, n_end) of the slot's incoming stream x (float32, as the incoming
// stage's source forms them) into `out`, sample e_new first -- sample n from old[n - base] below n_old (the half the push
// reads), from the caller's PCM at `in` from n_old on (fmt / ch / sum as ResampleRun's hb_fmt / hb_ch / hb_sum).  One
// workgroup per run; lanes read and write consecutive samples.
struct HoldRun {
    const float* old;
    float* out;
    const void* in;
    long long base, n_old, e_new, n_end;
    int fmt, ch, sum;
};
void launch_hold(const char* kernel, const HoldRun* runs_dev, int nruns, hipStream_t s);

// peak + normalise: blocks of <= kNormBlock samples; block b belongs to a clip whose blocks are [pb0, pb0 + pbn)
struct NormBlock {
    long long off;
    int n, pb0, pbn;
};
constexpr int kNormBlock = 8192;
void launch_peak_partial(const float* x, const NormBlock* blocks_dev, int nblocks, int wrap, float* partial, hipStream_t s);
void launch_peak_normalise(const float* x, const NormBlock* blocks_dev, int nblocks, const float* partial, float* out, hipStream_t s);
// out[i] = mean_c in[c * n + i] (channel-major planes of n samples; out may be plane 0)
void launch_channel_mean(const float* in, int nchan, int64_t n, float* out, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Level meter and automatic compensation (level.hip; include/nhans_hip.h: nhans_level_*).  One workgroup: the hops
// [hop_first, hop_first + nh) of one stream or clip -- hop h = samples [160 h, 160 h + 160), the last one of an ended
// stream shorter -- whose samples are at den / mix from sample 160 * hop_first on, n_new of them.  It writes one gain per
// hop to wtab and, where asked, the carried state and the meter.
// State of a stream, kLevelState doubles: [3][256] the powers Pd, Pr, Pm of the last <= 256 hops (hop j at j mod 256),
// [3] the running sums since hop h0, [8] the meter (nhans_level_live_read).
struct LevelRun {
    const float* den;
    const float* mix;
    const double* in;       // the state before hop_first; nullable: there is none (hop_first == h0)
    double* out;            // nullable: the state after the last hop is not kept
    double* meter;          // nullable: 8 doubles, the meter after the last hop
    float* wtab;            // nh gains
    long long n_new, hop_first, nh, h0;
    int W;                  // window in hops, 1 .. 256; 0: cumulative since h0
    double wmax;
};
constexpr int kLevelRing = 256, kLevelSums = 3 * kLevelRing, kLevelMeter = kLevelSums + 3, kLevelState = kLevelMeter + 8 + 5;
void launch_level(const char* kernel, const LevelRun* runs_dev, int nruns, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Filterbank features (fbank.hip; include/nhans_hip.h: nhans_fbank_*).  One run: nrows consecutive [201] log-magnitude
// rows at src -> nrows consecutive [n_out] rows at dst; its tiles of kFbankTile rows are workgroups [tile0, tile0 +
// ceil(nrows / kFbankTile)) of the launch, tile0 ascending from 0 over the runs (fbank_launch, host_fbank.hip, builds them).
// The band table on the device, 32-bit words: first[n_out], count[n_out], woff[n_out], then the nspan float32 weights,
// band m's at woff[m] .. woff[m] + count[m]; first[m] + count[m] <= 201.
struct FbankRun {
    const float* src;
    float* dst;
    long long nrows, tile0;
};
constexpr int kFbankTile = 16, kFbankMaxOut = 128, kFbankMaxSpan = 8192;
constexpr float kFbankMaxExponent = 88.f;       // p = expf(min(power * x, 88)): finite whatever the row holds
size_t fbank_lds_bytes(int n_out, int nspan);
void launch_fbank(const char* kernel, const FbankRun* runs_dev, int nruns, long long ntiles, const int* table_dev, int n_out,
                  int nspan, int power, float floor, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Scoring against a clean target (score.hip; include/nhans_hip.h: nhans_score_*).  One ScoreRun per clip pair, empty ones
// included: n common samples at est / tgt; its tiles of kScoreTile samples are workgroups [tile0, tile0 + ceil(n /
// kScoreTile)) of the two tile launches, its segments of kScoreSegment samples entries [seg0, seg0 + ceil(n /
// kScoreSegment)) of the segment powers, its frames rows [frame0, frame0 + frames) of the per-frame output; tile0, seg0
// and frame0 ascend from 0 over the runs.  One ScoreRowRun per pair of row tensors: frames rows of 201 at est / tgt, its
// tiles of kScoreRowTile rows workgroups [tile0, ...) of the rows launch.  The finish launches: one workgroup per run.
struct ScoreRun {
    const float* est;
    const float* tgt;
    long long n, tile0, seg0, frame0, frames;
};
struct ScoreRowRun {
    const float* est;
    const float* tgt;
    long long frames, tile0, frame0;
};
constexpr int kScoreSegment = 80, kScoreTile = 2560, kScoreRowTile = 16, kScoreFields = 16, kScoreRowFields = 8;
// part: [tiles][4] doubles (pass 2 writes column 0 only); segs: [segments][2] = Pt, Pd; rec: [runs][kScoreFields]
void launch_score_tiles(const char* kernel, int pass, const ScoreRun* runs_dev, int nruns, long long ntiles, double* part,
                        double* segs, const double* rec, hipStream_t s);
void launch_score_finish(const char* kernel, const ScoreRun* runs_dev, int nruns, const double* part, const double* segs,
                         double* rec, double* frames_out, hipStream_t s);
void launch_score_sisdr(const char* kernel, const ScoreRun* runs_dev, int nruns, const double* part, double* rec, hipStream_t s);
// vals: [rows][2] = loss_f, lsd_f; rec: [runs][kScoreRowFields]
void launch_score_rows(const char* kernel, const ScoreRowRun* runs_dev, int nruns, long long ntiles, double* vals,
                       double* frames_out, hipStream_t s);
void launch_score_rows_finish(const char* kernel, const ScoreRowRun* runs_dev, int nruns, const double* vals, double* rec,
                              hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Mixing at a chosen SNR (mix.hip; include/nhans_hip.h: nhans_mix).  One MixChain per DISTINCT (clip, fitted length):
// the mean square of the m samples at src fitted to n (sample i mod m where m < n, else sample i), one workgroup of
// mix_power each, -> pw[its index].  One MixJob per job: n samples of speech at s, the keep noise at a (ma samples;
// nullptr: the two-way mix) and the drop noise at b (mb), their chains' indices ps / pa / pb (pa unused without a), the
// host's factors fa / fb = pow(10, -snr / 10), its outputs from element `out` of every output buffer on and its tiles of
// kMixTile samples workgroups [tile0, tile0 + ceil(n / kMixTile)) of mix_combine and mix_finish (n >= 1, so tile0
// ascends strictly).  kMixTile is also what mix_power stages at a time.
struct MixChain {
    const float* src;
    long long m, n;
};
struct MixJob {
    const float* s;
    const float* a;
    const float* b;
    long long n, ma, mb, out, tile0;
    double fa, fb;
    int ps, pa, pb, pad;
};
constexpr int kMixTile = 2048, kMixFields = 8;
void launch_mix_power(const char* kernel, const MixChain* chains_dev, int nchains, double* pw, hipStream_t s);
// peaks: [tiles] floats, max |raw| of each tile; rec (nullable): [jobs][kMixFields], fields 0 - 4 written here
void launch_mix_combine(const char* kernel, const MixJob* jobs_dev, int njobs, long long ntiles, const double* pw, float* mixture,
                        float* peaks, double* rec, hipStream_t s);
// mixture divided in place; target / keep / drop nullable; fields 5 - 7 of rec
void launch_mix_finish(const char* kernel, const MixJob* jobs_dev, int njobs, long long ntiles, const double* pw, const float* peaks,
                       float* mixture, float* target, float* keep, float* drop, double* rec, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// STOI and extended STOI against a clean target (stoi.hip; include/nhans_hip.h: nhans_stoi).  One StoiRun per clip pair,
// empty ones included: n common samples at est / tgt (10 kHz) and `frames` = M0 frames of 256 at hop 128.  What a clip
// owns in the call's scratch is sized by n alone, since how many frames are silent is known on the device only: entries
// [frame0, frame0 + M0) of the frame powers and of the kept-frame list, rows [band0, band0 + max(M0 - 1, 0)) of the two
// band tensors, rows [seg0, seg0 + max(M0 - 30, 0)) of the segment figures; and workgroups [ptile0, ...) of the power
// launch (kStoiPowerTile frames each), [btile0, ...) of the band launch (kStoiBandTile analysis frames each) and
// [stile0, ...) of the segment launch (kStoiSegTile segments each).  All of them ascend from 0 over the runs.  A
// workgroup past what the clip really kept finds that in nkept[run] and leaves.
struct StoiRun {
    const float* est;
    const float* tgt;
    long long n, frames, frame0, band0, seg0, ptile0, btile0, stile0;
};
constexpr int kStoiFields = 8, kStoiFrame = 256, kStoiHop = 128, kStoiFft = 512, kStoiBands = 15, kStoiSegment = 30;
constexpr int kStoiPowerTile = 4, kStoiBandTile = 2, kStoiSegTile = 16;
constexpr int kStoiTable = kStoiFrame + 2 * kStoiFft;      // doubles: the window, then cos and -sin of 2 pi t / 512
inline long long stoi_frames(long long n) { return n > kStoiFrame ? (n - kStoiFrame + kStoiHop - 1) / kStoiHop : 0; }
void stoi_table(double* tab);                               // (host) the kStoiTable doubles
void launch_stoi_power(const char* kernel, const StoiRun* runs_dev, int nruns, long long ntiles, const double* tab, double* power,
                       hipStream_t s);
void launch_stoi_keep(const char* kernel, const StoiRun* runs_dev, int nruns, const double* power, int* kept, long long* nkept,
                      hipStream_t s);
// bands: [2][rows][15] doubles, the target's then the estimate's (the second half begins at row `rows`)
void launch_stoi_bands(const char* kernel, const StoiRun* runs_dev, int nruns, long long ntiles, const double* tab, const int* kept,
                       const long long* nkept, double* bands, long long rows, hipStream_t s);
// segs: [rows][2] = d_s, e_s; segs_out: the caller's copy, nullable
void launch_stoi_segments(const char* kernel, const StoiRun* runs_dev, int nruns, long long ntiles, const long long* nkept,
                          const double* bands, long long rows, double* segs, double* segs_out, hipStream_t s);
void launch_stoi_finish(const char* kernel, const StoiRun* runs_dev, int nruns, const long long* nkept, const double* segs,
                        double* rec, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// BSS Eval: SDR, SIR and SAR against target and interferer (bsseval.hip; include/nhans_hip.h: nhans_bss_eval).  One BssRun
// per clip of a group, empty ones included: n common samples at est / s0 / s1 (s1: nullptr with one source), workgroups
// [ctile0, ctile0 + ctiles) of the correlation launch (kBssCorrTile samples each; their partial sums are rows of the same
// numbers) and [ptile0, ptile0 + ptiles) of the projection launch (kBssProjTile samples of [0, n + L - 1) each; their
// partial energies likewise).  Both ascend from 0 over the runs.  L and J = 1 | 2 are the call's; NI = 6 sums of L lags
// with two sources (r00, r10, r01, r11, q0, q1), 2 with one (r00, q0); M = J L.
struct BssRun {
    const float* est;
    const float* s0;
    const float* s1;
    long long n, ctile0, ctiles, ptile0, ptiles;
};
constexpr int kBssFields = 16, kBssMaxL = 512, kBssCorrTile = 2048, kBssProjTile = 1024, kBssPanel = 16;
// part: [tiles][NI][L]
void launch_bss_corr(const char* kernel, const BssRun* runs_dev, int nruns, long long ntiles, int L, int J, double* part, hipStream_t s);
// lag: [clips][NI][L]
void launch_bss_reduce(const char* kernel, const BssRun* runs_dev, int nruns, int L, int J, const double* part, double* lag, hipStream_t s);
// G: [clips][M][M], column-major, the lower triangle written
void launch_bss_gram(const char* kernel, int nruns, int L, int J, const double* lag, double* G, hipStream_t s);
// G -> its factor in place; sol and filt (the caller's copy, nullable): [clips][M + L] = C, then C0; flag: [clips], 1 = singular
void launch_bss_chol(const char* kernel, int nruns, int L, int J, const double* lag, double* G, double* sol, double* filt, int* flag,
                     hipStream_t s);
// epart: [tiles][6] = the tile's part of E_e, E_tgt, E_int, E_art, E_dist, E_ti
void launch_bss_project(const char* kernel, const BssRun* runs_dev, int nruns, long long ntiles, int L, int J, const double* sol,
                        const int* flag, double* epart, hipStream_t s);
void launch_bss_finish(const char* kernel, const BssRun* runs_dev, int nruns, int L, int J, const int* flag, const double* epart, double* rec,
                       hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Delay estimation (align.hip; include/nhans_hip.h: nhans_align, nhans_align_cut).  One AlignRun per clip pair, empty ones
// included: ne samples at est, nt at tgt (a pointer is nullptr where its count is 0).  D = max_lag is the call's; a clip's
// lag vector is 2 D + 1 doubles, lag -D first.  align_corr: one workgroup per (clip, block of kAlignLagBlock lags), sample
// tiles of kAlignTile anchored at the target's first sample.  One AlignCopy per non-empty piece of the ragged copy: n > 0
// samples from src to dst, workgroups [tile0, tile0 + ceil(n / kAlignCutTile)), tile0 ascending strictly from 0.
struct AlignRun {
    const float* est;
    const float* tgt;
    long long ne, nt;
};
struct AlignCopy {
    const float* src;
    float* dst;
    long long n, tile0;
};
constexpr int kAlignFields = 8, kAlignMaxLag = 16000, kAlignTile = 2048, kAlignLagBlock = 2048, kAlignCutTile = 4096;
// corr: [clips][2 D + 1]
void launch_align_corr(const char* kernel, const AlignRun* runs_dev, int nruns, int D, double* corr, hipStream_t s);
// rec: [clips][kAlignFields]
void launch_align_pick(const char* kernel, const AlignRun* runs_dev, int nruns, int D, const double* corr, double* rec, hipStream_t s);
void launch_align_cut(const char* kernel, const AlignCopy* jobs_dev, int njobs, long long ntiles, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// LLR, cepstral distance and frequency-weighted segmental SNR against a clean target (quality.hip; include/nhans_hip.h:
// nhans_quality).  One QualityRun per clip pair, empty ones included: n common samples at est / tgt (16 kHz) and `frames`
// = M frames of 480 at hop 120.  A clip owns rows [frame0, frame0 + M) of the per-frame values and workgroups
// [ltile0, ...) of the LPC launch (kQualityLpcTile frames each) and [btile0, ...) of the band launch (kQualityBandTile
// frames each); all of them ascend from 0 over the runs.
struct QualityRun {
    const float* est;
    const float* tgt;
    long long n, frames, frame0, ltile0, btile0;
};
constexpr int kQualityFields = 16, kQualityFrame = 480, kQualityHop = 120, kQualityOrder = 16, kQualityFft = 512, kQualityBins = 257;
constexpr int kQualityBands = 25, kQualityMaxBands = 32, kQualityLpcTile = 7, kQualityBandTile = 2;
constexpr int kQualityLpcFields = 72;       // a frame's row of nhans_quality_lpc: r_t[17], r_e[17], a_t[17], a_e[17], num, den, dc2, 0
constexpr int kQualityTable = kQualityFrame + 2 * kQualityFft;      // doubles: the window, then cos and -sin of 2 pi t / 512
constexpr double kQualityLlrMax = 2.0, kQualityCdMax = 10.0, kQualityCdScale = 4.342944819032518 /* 10 / ln 10 */;
constexpr double kQualitySnrMin = -10.0, kQualitySnrMax = 35.0, kQualityGamma = 0.2;
inline long long quality_frames(long long n) { return n >= kQualityFrame ? (n - kQualityFrame) / kQualityHop + 1 : 0; }
void quality_table(double* tab);                            // (host) the kQualityTable doubles
void quality_default_bands(double* w);                      // (host) [kQualityBands][kQualityBins]
// vals: [frames][3] = llr_f, cd_f (this launch), fw_f (the band launch); lpc_out (nullable): [frames][kQualityLpcFields]
void launch_quality_lpc(const char* kernel, const QualityRun* runs_dev, int nruns, long long ntiles, const double* tab, double* vals,
                        double* lpc_out, hipStream_t s);
// bands: [nbands][kQualityBins]; span: [nbands][2] = the bins [first, last + 1) of each row's non-zero weights (0, 0: none)
void launch_quality_bands(const char* kernel, const QualityRun* runs_dev, int nruns, long long ntiles, const double* tab,
                          const double* bands, const int* span, int nbands, double* vals, hipStream_t s);
// rec: [clips][kQualityFields]
void launch_quality_finish(const char* kernel, const QualityRun* runs_dev, int nruns, const double* vals, double* rec, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Drift-aware alignment (drift.hip; include/nhans_hip.h: nhans_drift_track, nhans_drift_warp).  Target sample u lines up
// with position p(u) = a + u + b u of the estimate.  The interpolation table: G [kDriftQ + 1][2 kDriftT] then D [kDriftQ][2
// kDriftT] doubles, tap k = -kDriftT + 1 ... kDriftT at column k + kDriftT - 1.  One DriftSeg per tracked segment, in the
// order of the records: the block of kDriftBlock target samples at tgt (target sample u0 of its clip), the whole estimate
// (ne samples at est, nullptr where ne is 0) and the centre lag z; its lag vector is 2 (R + kDriftT) + 1 doubles, lag
// z - R - kDriftT first.  One DriftWarp per clip with a non-empty range: outputs [u_lo, u_lo + n) to dst, workgroups [tile0,
// tile0 + ceil(n / kDriftWarpTile)), tile0 ascending strictly from 0.
struct DriftSeg {
    const float* est;
    const float* tgt;
    long long ne, u0;
    int z, pad;
};
struct DriftWarp {
    const float* est;
    float* dst;
    long long ne, u_lo, n, tile0;
    double a, b;
};
constexpr int kDriftFields = 8, kDriftFitFields = 6, kDriftT = 16, kDriftQ = 512, kDriftBlock = 4096, kDriftHop = 2048, kDriftMaxR = 1024;
constexpr int kDriftTile = 2048;            // samples per fma chain of a lag sum (the tile of align.hip)
constexpr int kDriftFine = 32;              // fine positions per sample of the peak search
constexpr int kDriftWarpTile = 1024;        // outputs per workgroup of the warp
constexpr int kDriftTableG = (kDriftQ + 1) * 2 * kDriftT, kDriftTableD = kDriftQ * 2 * kDriftT;
constexpr double kDriftMaxSlope = 0.0009765625;     // 2^-10
constexpr double kDriftMaxDelay = 2147483648.0;     // |a| <= 2^31: p(u) stays strictly increasing in u, rounding included
inline long long drift_segments(long long nt) { return nt >= kDriftBlock ? (nt - kDriftBlock) / kDriftHop + 1 : 0; }
// p(u), the one expression of the device and of nhans_drift_range: fma(b, u, a) rounded, then + u rounded
__host__ __device__ inline double drift_pos(double a, double b, double u) {
#pragma clang fp contract(off)
    const double f = __builtin_fma(b, u, a);
    return f + u;
}
void drift_table(double* g, double* d);                      // (host) kDriftTableG and kDriftTableD doubles
// tab: G then D on the device; rec: [segments][kDriftFields]; corr (nullable): [segments][2 (R + kDriftT) + 1]
void launch_drift_track(const char* kernel, const DriftSeg* segs_dev, int nsegs, int R, const double* tab, double* rec, double* corr,
                        hipStream_t s);
void launch_drift_warp(const char* kernel, const DriftWarp* jobs_dev, int njobs, long long ntiles, const double* tab, hipStream_t s);

}  // namespace nhans
