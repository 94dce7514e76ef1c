// What the host units of libnhans_hip.so share (the C ABI itself: include/nhans_hip.h).  One unit per subsystem:
//   ws_plan.h         WsPlan: a call's device scratch, each buffer declared once (knows neither HIP nor the context)
//   net_weights.h     NetWeights: the blob's arrays, each declared once with its size and class and resolved into one field
//                     (knows neither HIP nor the context); BlockGeo and the two geometries
//   host_ctx.hip      error channel, blob (nhans_create_ex checks it: resolve_net_weights), context, options, calibration,
//                     workspace growth and ws_commit, Call, status, profiling, the argument checks several units share
//   host_net.hip      conv launch sequences (tower, stack, head), STFT / iSTFT block tables, the offline entry points
//   host_fbank.hip    filterbank design and table, nhans_fbank_design / _open / _close / _rows
//   host_online.hip   nhans_online_*, nhans_capture_*, nhans_fbank_online_*
//   host_rate.hip     rate-conversion stages, nhans_resample*, nhans_peak_normalise, nhans_channel_mean, nhans_resampler_*
//   host_live.hip     nhans_live_*, nhans_lookahead_live_*, nhans_capture_live_*, nhans_level_*, nhans_interleaved_*,
//                     nhans_fbank_live_*, nhans_fullband_*
//   host_score.hip    nhans_score_wave, nhans_score_rows
//   host_mix.hip      nhans_mix, nhans_mix_snr_factor
//   host_stoi.hip     nhans_stoi, nhans_stoi_resample, nhans_stoi_out_count
//   host_bsseval.hip  nhans_bss_eval
//   host_align.hip    nhans_align, nhans_align_common, nhans_align_cut
//   host_quality.hip  nhans_quality, nhans_quality_lpc, nhans_quality_tables
//   host_drift.hip    nhans_drift_table, nhans_drift_segments, nhans_drift_range, nhans_drift_fit, nhans_drift_track, nhans_drift_warp
//   host_phase.hip    nhans_phase_project, nhans_phase_refine, nhans_phase_set_alpha; the refinement inside nhans_enhance_clips
// A unit calls down only: ctx <- net <- online <- live, ctx <- fbank <- online, ctx <- rate <- live, ctx <- score, ctx <- mix, ctx <- rate <- stoi, ctx <- bsseval, ctx <- align, ctx <- quality, ctx <- drift and ctx <- phase <- net.  (One call goes up: the built-in calibration
// of nhans_create runs the whole offline path, enhance_clips_body.)  Only what crosses a unit boundary is declared here;
// everything else stays in its unit's anonymous namespace.
// Nothing declared here joins the library's dynamic symbols (visibility hidden) except the object types the C header
// names, which keep the default visibility they have always had.
#pragma once
#include "../../include/nhans_hip.h"
#include "nhans_kernels.h"
#include "ws_plan.h"
#include "net_weights.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <string>
#include <vector>

using namespace nhans;

#pragma GCC visibility push(hidden)

// ---- host_ctx.hip ---------------------------------------------------------------------------------
int fail(int code, const std::string& msg);       // sets nhans_last_error() (thread-local), returns code

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(NHANS_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

constexpr int kNumAct = NHANS_NUM_ACTIVATIONS;
constexpr int TA(int b, int j) { return 2 * b + j; }            // tower block b, conv j+1
constexpr int SA(int b, int j) { return 8 + 2 * b + j; }        // stack block b, conv j+1
constexpr int kActHead = 24;                                    // last_conv

struct ProfEntry {
    int calls = 0;
    double flops = 0, bytes = 0, mfma = 0;      // algorithmic FLOPs / bytes; FLOPs the matrix cores executed
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0;
};

#pragma GCC visibility pop

// which convs of the stack ran in their Winograd form in the last chunk (run_stack_chunk)
struct StackPlan {
    bool wino[8][3] = {};      // [block][conv 1 | 2]
};

struct nhans_ctx {
    int kind = 0, device = 0;
    StackPlan last_plan;
    float* blob_dev = nullptr;
    size_t blob_bytes = 0;
    NetWeights net;         // the blob's arrays on the device (net_weights.h), resolved and checked by nhans_create_ex
    std::vector<BlockGeo> tower, stack;
    int cond_cols = 0;
    std::vector<int> cond_off;      // column offset of conv j (= 2*block + {0,1})
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    // split-K scratch of the conv kernel (small launches only)
    // Allocated LAZILY, sized by the launches that actually split (run_conv: conv_splitk_scratch_bytes) and grown up to
    // 96 tiles x 32 groups x 128 KB = 384 MB, all the split-K rule of conv_igemm_dma.hip admits (round-5 advisor: 384 MB
    // taken unconditionally at nhans_create was 3 GB for eight ranks sharing a device, and its failure failed the
    // create).  A failed allocation is not an error: the launch walks its groups unsplit -- same bits, fewer CUs.
    float* kscratch = nullptr;
    size_t kscratch_bytes = 0;
    static constexpr size_t kscratch_cap = (size_t)384 << 20;
    bool kscratch_failed = false;
    int stream_1x1 = 1;         // option stream_1x1: the stand-alone `_transform` conv on conv_1x1_stream.hip (0: the generic conv kernel; same bits)
    int row_split = 1;          // option row_split: convs on small images as one launch per row class (host_net.hip: run_conv_row_classes; 0: one launch; same bits)
    int split_k = 1;            // option split_k: 0 = never split (the grouped walk inside one workgroup: same bits)
    int* kcounter = nullptr;
    int kcounter_n = 1024;
    // Frame windows per pass of the stack.  Every launch runs whole "waves" of one workgroup per CU and all
    // workgroups of a launch take the same time, so a launch whose tile count is not a multiple of 256
    // leaves CUs idle for a tile time at its end: 1,024 frames give resblock4 (130 pixels per frame, 256-pixel
    // x 4 channel tiles) 8.1 waves = 9.7 % lost, 3.9 % over the whole stack.  3,776 = 59 x 64 frames minimise
    // the FLOP-weighted loss (0.18 %) among the sizes whose largest tensor (3,776 x 35 x 201 x 64 elements)
    // still fits the kernels' 32-bit element offsets; the three ping-pong buffers are then 20 GB of the 288.
    int64_t frames_per_chunk = 3776;
    int contexts_per_chunk = 64;
    size_t bss_group_bytes = (size_t)2 << 30;   // option bss_group_bytes: the factor storage one group of nhans_bss_eval's clips may take (host_bsseval.hip; same bits)
    int lookahead = kCenter;    // option lookahead: frame t of a clip sees the clip end at min(len, t + lookahead + 1) (offline calls)
    int phase_iters = 0;        // option phase_iters: Griffin-Lim iterations of nhans_enhance_clips between mask net and iSTFT (0: none)
    double phase_alpha = 0.0;   // nhans_phase_set_alpha: their momentum
    // pinned staging ring for the small host tables (offsets, block lists) copied per call
    char* pin = nullptr;
    size_t pin_bytes = (size_t)16 << 20, pin_top = 0;
    // profiling
    bool profile = false;
    std::map<std::string, ProfEntry> prof;
    std::vector<hipEvent_t> event_pool;

    int prec = 0;           // 0: f32 MFMA, 1: split-f16 x3 MFMA (activations in split NHWC)
    int conv_variant = -1;  // 0: 128-pixel register-staged conv kernel, 1: 256-pixel LDS-DMA kernel,
                            // 2: halo-reuse / wave-specialised LDS-DMA kernel where the conv allows it, else 1;
                            // -1: automatic (measured best: 2 for split-f16, register-staged for f32)
    int epi8 = 1;               // ConvArgs::epi8
    int ilv = 1;                // ConvArgs::ilv
    int wino = 1;               // ConvArgs::wino: 1-D Winograd form of the stride-1 stack convs (conv_wino.hip)
    int wino_f32 = 1;           // tensors that only Winograd launches read are stored f32 NHWC (stored_f32())
    long long* dbg = nullptr;   // NHANS_DEV builds: per-workgroup cycle stamps of the last conv launch
    int* status_dev = nullptr;  // sticky NHANS_STATUS_* bits set by kernels (nhans_take_status)
    std::map<std::pair<int, int>, float*> rs_tab;   // device copies of the rate converter's phase tables, by (rate_in, rate_out)
    double* drift_tab = nullptr;    // device copy of the drift interpolation table, G then D (host_drift.hip: designed at its first use)
    // Activation exponents: a split-f16 tensor is stored as x * 2^-e with one e per tensor of the network, chosen from
    // the largest |x| a calibration pass saw so that the stored maximum is <= 2^kActTargetLog2 -- 2^8 below the f16
    // limit (and the 1-D Winograd transform's worst-case gain of ~20 still fits).  Tensors: tower block b conv1/conv2
    // outputs (2b, 2b+1), stack block b conv1/conv2 outputs (8+2b, 8+2b+1), last_conv output (24).  f32 tensors carry
    // no exponent.  The flag of nhans_take_status stays as the backstop for inputs far outside the calibration.
    int act_exp[kNumAct] = {};
    float act_amax[kNumAct] = {};       // what the last calibration saw (diagnostics)
    unsigned* amax_dev = nullptr;       // running maxima (float bits) while calibrating
    bool calibrating = false;
    // debug capture (nhans_debug_activation / nhans_debug_tower_activation): the tensor whose finished buffer the tap()
    // points of the production launch sequences copy out as plain f32 NHWC, chunk after chunk; -1: none (every other call)
    int cap_idx = -1;
    float* cap_out = nullptr;
    float up(int i) const { return prec ? ldexpf(1.f, act_exp[i]) : 1.f; }
    float down(int i) const { return prec ? ldexpf(1.f, -act_exp[i]) : 1.f; }
    // ordering of consecutive calls that share the workspace (see include/nhans_hip.h)
    hipEvent_t tail_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_tail = false;
};

#pragma GCC visibility push(hidden)

// A call's scratch: declare every buffer in a WsPlan (ws_plan.h), then commit -- the workspace grows to the plan's bytes
// if it has to (synchronise, free, allocate) and every declared pointer is placed in it, from offset 0.  One call may
// commit several plans in sequence: each takes the workspace from offset 0 again, and stream order makes that safe.
int ws_commit(nhans_ctx* c, const WsPlan& p);
// Host -> device copy of a small table through the pinned ring, so the caller's (pageable, soon
// destroyed) buffer is never the source of an in-flight asynchronous copy.
int h2d(nhans_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t s);
// a whole host table to the device array of its element type
template <typename T> int h2d(nhans_ctx* c, T* dst, const std::vector<T>& v, hipStream_t s) {
    return h2d(c, dst, v.data(), v.size() * sizeof(T), s);
}

// The plan of a call whose only scratch is one host table: room for it, and its copy on s.
template <typename T> int ws_upload(nhans_ctx* c, const std::vector<T>& v, hipStream_t s, T** dev) {
    WsPlan p;
    p.add(dev, v.size());
    const int rc = ws_commit(c, p); if (rc) return rc;
    return h2d(c, *dev, v, s);
}

// RAII-less profiling bracket around one launch
struct Prof {
    nhans_ctx* c;
    hipStream_t s;
    ProfEntry* e = nullptr;
    hipEvent_t a{}, b{};
    static hipEvent_t take(nhans_ctx* c) {
        hipEvent_t ev = nullptr;
        if (!c->event_pool.empty()) { ev = c->event_pool.back(); c->event_pool.pop_back(); }
        else (void)hipEventCreate(&ev);
        return ev;
    }
    Prof(nhans_ctx* c_, hipStream_t s_, const char* name) : c(c_), s(s_) {
        if (!c->profile) return;
        if (name) e = &c->prof[name];
        a = take(c);
        b = take(c);
        (void)hipEventRecord(a, s);
    }
    void done(double flops, double bytes, const char* late_name = nullptr, double mfma = 0) {
        if (!c->profile) return;
        if (late_name) e = &c->prof[late_name];
        if (!e) return;
        (void)hipEventRecord(b, s);
        e->pending.emplace_back(a, b);
        e->calls += 1;
        e->flops += flops;
        e->bytes += bytes;
        e->mfma += mfma;
    }
};

int check_ctx(nhans_ctx* c);
// A launch the runtime rejected anywhere in the sequence just issued -> NHANS_EHIP.
int launch_status();

// Bracket of one stream-taking entry point: selects the device, orders the call behind the previous
// call on this context when that one ran on another stream (they share workspace, pinned tables
// and split-K tickets), and on the way out collects launch failures and marks the new tail.
// Nothing of it is public: bracket_call below is the only code that can open or close one, and the entry points
// reach it through ctx_call, object_call and object_count_call -- a body cannot return past the way out.
class Call {
    nhans_ctx* c;
    hipStream_t s;
    int rc;
    Call(nhans_ctx* c_, void* stream);
    int finish(int body_rc);
    template <typename Body> friend int64_t bracket_call(nhans_ctx* c, void* stream, Body body);
};

// body(stream) inside the Call.  What the body returns is a status (negative: every code but NHANS_OK is) or a count
// (>= 0; NHANS_OK is the count 0), and so is what comes back: the first of the Call's own refusal, the body's status and
// a failed launch -- else the body's count.
template <typename Body>
int64_t bracket_call(nhans_ctx* c, void* stream, Body body) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    const int64_t n = body(call.s);
    const int rc = call.finish(n < 0 ? (int)n : NHANS_OK);
    return rc ? rc : n;
}

// The bracket for an entry point of the context itself; its body returns a status.
template <typename Body>
int ctx_call(nhans_ctx* c, void* stream, Body body) {
    return (int)bracket_call(c, stream, body);
}

// The bracket for an entry point of an object that holds its context (nhans_online, nhans_resampler, nhans_live,
// nhans_fbank): the null check with the entry point's own message first.  object_count_call: the body returns an
// int64_t, a count or a negative status.
template <typename Obj, typename Body>
int64_t object_count_call(Obj* o, const char* null_msg, void* stream, Body body) {
    if (!o) return fail(NHANS_EINVAL, null_msg);
    return bracket_call(o->c, stream, body);
}
template <typename Obj, typename Body>
int object_call(Obj* o, const char* null_msg, void* stream, Body body) {
    return (int)object_count_call(o, null_msg, stream, body);
}

// argument checks the streaming objects share
int slot_check(int S, int slot, const char* fn);
constexpr int64_t kMaxResampleClip = ((int64_t)1 << 31) - 1, kNoPushCap = std::numeric_limits<int64_t>::max();
int push_check(const char* fn, const char* noun, int i, int64_t cnt, bool en, bool ended, const char* uncond, int64_t max_cnt);
// the nclips + 1 offsets `off` (`what`: which ones, for the message) do not descend
int offsets_check(const std::string& fn, const char* what, const int64_t* off, int nclips);
// What the calls on (est, eoff, tgt, toff, nclips, out) refuse before they look at a clip -- a negative count, null
// offsets or output (`verb`: what the call does to clips, for the message), descending offsets --, then body(i, e, t, ne,
// nt) for clip after clip: its first samples in the two buffers (nullptr where the buffer is) and its two lengths.  The
// body keeps its call's own caps and its run-table line; the first status that is not NHANS_OK ends the walk.
using PairBody = std::function<int(int i, const float* e, const float* t, int64_t ne, int64_t nt)>;
int pair_clips(const std::string& fn, const char* verb, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff,
               int nclips, const void* out, const PairBody& body);
int null_clip(const std::string& fn, int i, int64_t n);        // the refusal of clip i: n samples and a null buffer

// ---- host_phase.hip -------------------------------------------------------------------------------
// The scratch of a refinement of `total` frames in nclips clips, declared once: the A plane, two state planes, the d
// plane (momentum only), the frame partials, the tables.  phase_refine_run issues the launches of iters >= 1 iterations
// from phase_in to phase_out (may be the same rows); inc_out (nullable): [nclips][iters] doubles.
struct PhaseBufs {
    float *A, *t[2], *d;
    double *num, *den;
    int64_t* foff_dev;
    int* blocks;
    size_t nblocks;
};
void phase_plan(WsPlan& p, const int64_t* foff, int nclips, bool momentum, PhaseBufs* pb);
int phase_refine_run(nhans_ctx* c, const float* logmag, const float* phase_in, const int64_t* foff, int nclips, int iters, double alpha,
                     float* phase_out, double* inc_out, const PhaseBufs& pb, hipStream_t s);

// ---- host_net.hip ---------------------------------------------------------------------------------
struct StackBufs {
    int* f_clip; int* f_t; int* f_T; int64_t* foff_dev; float* cb_all;
    float* X; float* A; float* Y;
    float* T;       // f32 output of a block's 1x1 `_transform` conv when its conv2 runs in Winograd form
};
void stack_plan(WsPlan& p, const nhans_ctx* c, int64_t total, int nclips, int64_t wf, StackBufs* sb);
struct TowerBufs {
    float *X, *A, *Y;       // the embedding tower's three ping-pong buffers, contexts_per_chunk images each
};
void tower_plan(WsPlan& p, const nhans_ctx* c, TowerBufs* tb);
size_t stft_blocks(const int64_t* soff, int nclips, int maxf);
size_t istft_blocks(const int64_t* foff, int nclips);
int stft_impl(nhans_ctx* c, const float* wav, const int64_t* soff, int nclips, int maxf, float* logmag,
              float* phase, int64_t* dev_tables /*3*(nclips+1)*/, int* dev_blocks, std::vector<int64_t>* foff_out,
              hipStream_t s, const char* prof_name = nullptr);
int istft_impl(nhans_ctx* c, const float* logmag, const float* phase, const int64_t* foff, int nclips,
               const int64_t* ooff, float* wav_out, int64_t* dev_tables, int* dev_blocks, hipStream_t s,
               const char* prof_name = "istft_ola");
int embed_impl(nhans_ctx* c, const float* ctx_lm, int n, float* emb_out, const TowerBufs& tb, hipStream_t s);
int mask_net_run(nhans_ctx* c, const float* win_src, const int* rb, const float* centre, int64_t total, int nclips,
                 const float* ea, const float* eb, float* logits, float* denoised, const StackBufs& sb, int64_t wf,
                 hipStream_t s);
int enhance_clips_body(nhans_ctx* c, const float* mix, const int64_t* moff, int nclips, const float* ca,
                       const int64_t* caoff, const float* cbw, const int64_t* cboff, float* den_wav,
                       float* mixed_wav, float* logmag_out, float* phase_out, float* logits_out, float* emb_out,
                       hipStream_t s);

// ---- host_fbank.hip --------------------------------------------------------------------------------
// A filterbank as the kernel reads it (nhans_kernels.h: the band table) with its device copy.  The host words are kept:
// nhans_fbank_online_attach copies the table into the online object from them, so the filterbank it came from may go.
struct FbankTable {
    int n_out = 0, power = 2, nspan = 0;
    float floor = 0.f;
    std::vector<int32_t> words;     // 3 * n_out + nspan
    int* dev = nullptr;
};
// a copy of `from` with a device table of its own (one hipMalloc, one synchronous copy); on failure nothing is allocated
int fbank_table_clone(const FbankTable& from, const char* fn, FbankTable* out);
void fbank_table_free(FbankTable* t);
// One launch `name` over runs of rows (src, dst, nrows each; tile0 is filled in here), through runs_dev: room for nruns.
struct FbankRows {
    const float* src;
    float* dst;
    int64_t nrows;
};
int fbank_launch(nhans_ctx* c, const FbankTable& t, const char* name, const FbankRows* rows, int nruns, FbankRun* runs_dev,
                 hipStream_t s);

#pragma GCC visibility pop

struct nhans_fbank {
    nhans_ctx* c = nullptr;
    int device = 0;
    FbankTable t;
};

#pragma GCC visibility push(hidden)

// ---- host_online.hip (the layout of a slot's state: there) -------------------------------------------
constexpr int kOnRows = 2 * kCenter + kIstftHopsPerBlock - 14;  // 42 >= 17 + 24
constexpr int kOnDenRows = kIstftHopsPerBlock + 2;              // 24
constexpr size_t kOnSamp = 0, kOnLm = kWin, kOnPh = kOnLm + (size_t)kOnRows * kBins, kOnDen = kOnPh + (size_t)kOnRows * kBins;
constexpr size_t kOnSlot = (kOnDen + (size_t)kOnDenRows * kBins + 63) & ~(size_t)63;   // 22,144 floats = 88.6 KB
struct OnStream {
    int64_t N = 0, T = 0;
    bool ended = false;
};

#pragma GCC visibility pop

struct nhans_online {
    nhans_ctx* c = nullptr;
    int device = 0, S = 0;
    bool mixed = false;
    float* emb = nullptr;       // [2S, 512]: a-rows then b-rows
    float* state = nullptr;     // [2][S][kOnSlot]
    int cur = 0;
    std::vector<OnStream> st, prev;
    std::vector<char> cond;     // slot has conditioning (nhans_online_open: all; nhans_online_open_slots: none yet)
    std::vector<int> la;        // slot's look-ahead L (nhans_online_set_lookahead; survives a restart, as conditioning does)
    bool can_rewind = false;
    // nhans_capture_enable: per slot the last kCaptureSamples samples pushed, sample k at position k mod kCaptureSamples
    // (nullptr until enabled), and vlo: the oldest sample of the slot's current timeline the ring still holds.  The ring is
    // not double-buffered as `state` is, so vlo only moves forward with what a push writes -- a rewound push has written too
    // -- and goes back only where a new timeline starts (restart: 0) or the ring does (enable: N).
    float* ring = nullptr;      // [S][kCaptureSamples]
    std::vector<int64_t> vlo, whi;  // whi: how far a push has written the slot's timeline (> N after a rewind; for messages)
    // nhans_fbank_online_attach: the object's own copy of a filterbank and the feature rows of the last push -- plane 0
    // (the denoised rows) at rows [0, F) of `rows`, plane 1 (the centre rows; `mixed` only) at [F, 2 F), slot i's at
    // off[i] .. off[i] + cnt[i] of each plane, frames first[i] on.  cnt is all zero where there is nothing to read.
    struct Fbank {
        bool on = false, mixed = false;
        FbankTable t;
        float* rows = nullptr;
        size_t cap = 0;             // (floats)
        int64_t F = 0;
        std::vector<int64_t> off, cnt, first;
        void forget() { std::fill(cnt.begin(), cnt.end(), 0); }
    } fb;
    float* slot(int k, int i) const { return state + ((size_t)k * S + i) * kOnSlot; }
};

#pragma GCC visibility push(hidden)

int64_t on_emitted(int64_t T, bool ended, int L);
int64_t online_emit_count(const nhans_online* o, int i, int64_t cnt, bool en);
void online_undo(nhans_online* o);
int online_open_slots_body(nhans_ctx* c, int S, int want_mixed, hipStream_t s, nhans_online** out);
void online_restart_slot(nhans_online* o, int slot);
int online_set_context_body(nhans_online* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb_,
                            hipStream_t s, int64_t* first_frame);
int online_set_embeddings_body(nhans_online* o, int slot, const float* ea, const float* eb, hipStream_t s, int64_t* first_frame);
int online_push_body(nhans_online* o, const float* in, const int64_t* inoff, const int* end, float* den_out,
                     float* mix_out, const int64_t* outoff, int64_t* counts, hipStream_t s);
int capture_enable_body(nhans_online* o, const char* fn, hipStream_t s);
int capture_context_body(nhans_online* o, const char* fn_, int n, const int* slots, const int* which, int flags,
                         hipStream_t s, int64_t* first_frame);
int capture_embeddings_body(const nhans_online* o, const char* fn, int slot, float* ea, float* eb, hipStream_t s);
int fbank_attach_body(nhans_online* o, const char* fn, const nhans_fbank* fb, int flags);
int64_t fbank_read_body(nhans_online* o, const char* fn, int slot, int plane, float* out, int64_t cap_rows, int64_t* first_frame,
                        hipStream_t s);

// ---- host_rate.hip (rs_table and rs_add_runs: RateStage's inline members call them) -----------------------
int rs_table(nhans_ctx* c, const ResampleFilter* f, const float** tab);
inline size_t rs_elem(int fmt) { return fmt == kResampleInt16 ? 2 : 4; }
void rs_add_runs(std::vector<ResampleRun>& runs, size_t* lds, const ResampleFilter& f, const void* src, const float* mix,
                 const float* hist, char* dst, size_t elem, float* hist_out, int64_t k0, int n_new, int64_t m_begin, int64_t m_end);

// what the kernel reads and stores (launch_resample): PCM of pcm_format -> float32, or the wet/dry mix -> PCM of pcm_format
struct RateIo {
    bool from_mix;
    int pcm_format, quantise;
    float wet;
    double factor;
    bool auto_wet = false;      // from_mix: each hop's factor comes from the runs' gain table (GainTab) instead of `wet`
    bool interleaved = false;   // the PCM side is frames of several channels (Interleave): the kernel's interleaved source / sink
    bool highband = false;      // from_mix: the full-band source and sink, on what HighBandIo puts into the runs
    size_t in_elem() const { return from_mix ? 4 : rs_elem(pcm_format); }
    size_t out_elem() const { return from_mix ? rs_elem(pcm_format) : 4; }
};

// What a streaming converter carries: the filter, its device table, the carried samples and per stream how far it is.
struct RateStage {
    const ResampleFilter* f = nullptr;
    const float* tab = nullptr;
    int S = 0;
    // [2][S][J]: the J samples before each stream's next one; cur[i] = the half that holds them.  A push reads half cur[i]
    // and writes the other one; the NEXT push reads what this one wrote and overwrites what it read.  That is race-free
    // because consecutive calls on a context are ordered on the device (same stream, or Call's tail event across streams).
    // A rewind is therefore host-only: the half of before the push is intact, and restore() points at it again.
    float* hist = nullptr;
    struct Streams {
        std::vector<int64_t> N;         // samples taken per stream
        std::vector<char> ended, cur;
    } st;
    struct Span { int64_t Eo, En; };    // outputs [Eo, En) of a stream

    int alloc(nhans_ctx* c, const char* fn, const ResampleFilter* filter, int nstreams) {
        const int rc = rs_table(c, filter, &tab); if (rc) return rc;
        f = filter; S = nstreams;
        st.N.assign(S, 0); st.ended.assign(S, 0); st.cur.assign(S, 0);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&hist), (size_t)2 * S * f->J * 4);
        if (e != hipSuccess) return fail(NHANS_ENOMEM, std::string(fn) + ": hipMalloc failed: " + hipGetErrorString(e));
        return NHANS_OK;
    }
    void release() { if (hist) (void)hipFree(hist); hist = nullptr; }
    float* h(int k, int i) const { return hist + ((size_t)k * S + i) * f->J; }
    // what cnt more samples (en: and the end) make final of stream i
    Span plan(int i, int64_t cnt, bool en) const {
        return {resample_emitted(*f, st.N[i], st.ended[i]), resample_emitted(*f, st.N[i] + cnt, st.ended[i] || en)};
    }
    // the runs of such a push, its cnt samples at src (mix: see ResampleRun), outputs e stored from dst on
    void add_runs(std::vector<ResampleRun>& runs, size_t* lds, int i, const void* src, const float* mix, char* dst, size_t elem,
                  int64_t cnt, Span e) const {
        if (cnt == 0 && e.En == e.Eo) return;
        rs_add_runs(runs, lds, *f, src, mix, h(st.cur[i], i), dst, elem, cnt > 0 ? h(1 - st.cur[i], i) : nullptr, st.N[i], (int)cnt,
                    e.Eo, e.En);
    }
    void commit(int i, int64_t cnt, bool en) {
        st.N[i] += cnt;
        st.ended[i] = st.ended[i] || en;
        if (cnt > 0) st.cur[i] = 1 - st.cur[i];
    }
    // (nothing is cleared on the device: a stream of 0 samples reads none of the carried ones -- their absolute index is negative)
    void restart(int i) { st.N[i] = 0; st.ended[i] = 0; }
    Streams save() const { return st; }
    void restore(const Streams& saved) { st = saved; }
};

// The per-hop wet factors of a live push (level.hip wrote them): slot i's begin at w[off[i]], its first one being that of
// the first hop the push makes final, hop N / 160 of a stream that had N samples.
struct GainTab {
    const float* w;
    const int64_t* off;
};

// The PCM side of a stage (io.interleaved) as frames of `ch` channels: stream i's first sample is element base[i] of the
// PCM buffer -- its piece's first frame, plus the channel it owns -- and it sums (incoming stage) or writes (outgoing stage)
// `n` channels from there on in every frame.  The stage's other side stays mono, at its offsets.
struct Interleave {
    int ch, n;
    const int64_t* base;
};

// The input's own band of a full-band live push (io.highband; ResampleRun's hb_ fields), per stream i of the outgoing
// stage: its gain, the hold half that has its incoming samples [base[i], n_old[i]), and the push's cnt[i] new ones --
// element pos[i] of the PCM at `in` on, laid out as the incoming stage read them (ch == 0: mono).
struct HighBandIo {
    const float* gain;
    const float* const* hold;
    const int64_t *base, *n_old, *cnt, *pos;
    const void* in;
    int fmt, ch, sum;
    double denom;
};
// the fields of one run whose first output is output m0 of its stream
inline void highband_run(ResampleRun& r, float gain, const float* hold, int64_t base, int64_t n_old, int64_t cnt, const void* in,
                         int fmt, int ch, int sum, double denom, int64_t m0) {
    r.hb_gain = gain; r.hb_hold = hold; r.hb_in = in;
    r.hb_base = base; r.hb_n_old = n_old; r.hb_n_end = n_old + cnt; r.hb_m0 = m0;
    r.hb_denom = denom; r.hb_fmt = fmt; r.hb_ch = ch; r.hb_sum = sum;
}

int stage_push(nhans_ctx* c, RateStage& g, const char* kernel, const RateIo& io, const void* in, const float* mix,
               const int64_t* inoff, const int* end, void* out, const int64_t* outoff, int64_t* counts, hipStream_t s,
               const GainTab* gains = nullptr, const Interleave* il = nullptr, const HighBandIo* hb = nullptr);
int rs_launch(nhans_ctx* c, const char* name, const std::vector<ResampleRun>& runs, const float* tab, const ResampleFilter& f,
              const RateIo& io, size_t lds, double in_bytes, double out_bytes, int64_t out_samples, hipStream_t s);

#pragma GCC visibility pop
