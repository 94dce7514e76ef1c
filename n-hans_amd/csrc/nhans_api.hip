// C ABI of libnhans_hip.so (see include/nhans_hip.h): context, folded-weight blob, workspace and
// the launch sequences of the N-HANS hot path.
#include "../../include/nhans_hip.h"
#include "nhans_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

using namespace nhans;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(NHANS_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// ---- folded blob -----------------------------------------------------------------------------
constexpr uint32_t kBlobVersion = 2;   // fold.py: BLOB_VERSION
struct BlobHeader {
    char magic[8];          // "NHANSFW1"
    uint32_t version;
    uint32_t n_entries;
    uint64_t total_bytes;
};
struct BlobEntry {
    char name[48];
    uint64_t offset;        // bytes from blob start, 256-byte aligned
    uint64_t nfloats;
};

struct BlockGeo {
    int kh, kw, sh, sw, cin, cout, hin, win, hout, wout;
};

void same_pad(int n, int k, int s, int* out, int* before) {
    *out = (n + s - 1) / s;
    int total = std::max((*out - 1) * s + k - n, 0);
    *before = total / 2;
}

std::vector<BlockGeo> tower_geometry() {       // SN/main.py:194-198
    const int kh[4] = {8, 8, 4, 4}, kw[4] = {4, 4, 4, 4}, sh[4] = {3, 3, 1, 1}, sw[4] = {2, 2, 1, 2};
    const int co[4] = {64, 128, 256, 512};
    std::vector<BlockGeo> v;
    int h = kCtxFrames, w = kBins, c = 1;
    for (int i = 0; i < 4; ++i) {
        BlockGeo g{kh[i], kw[i], sh[i], sw[i], c, co[i], h, w, (h + sh[i] - 1) / sh[i], (w + sw[i] - 1) / sw[i]};
        v.push_back(g);
        h = g.hout; w = g.wout; c = g.cout;
    }
    return v;
}

std::vector<BlockGeo> main_geometry() {        // SN/main.py:221-229
    const int k[8] = {4, 4, 4, 4, 3, 3, 3, 3}, s[8] = {1, 1, 2, 1, 2, 1, 2, 1};
    const int co[8] = {64, 64, 128, 128, 256, 256, 512, 512};
    std::vector<BlockGeo> v;
    int h = kMixWin, w = kBins, c = 1;
    for (int i = 0; i < 8; ++i) {
        BlockGeo g{k[i], k[i], s[i], s[i], c, co[i], h, w, (h + s[i] - 1) / s[i], (w + s[i] - 1) / s[i]};
        v.push_back(g);
        h = g.hout; w = g.wout; c = g.cout;
    }
    return v;
}

constexpr int kNumAct = NHANS_NUM_ACTIVATIONS;
constexpr int kActTargetLog2 = 8;
constexpr int TA(int b, int j) { return 2 * b + j; }            // tower block b, conv j+1
constexpr int SA(int b, int j) { return 8 + 2 * b + j; }        // stack block b, conv j+1
constexpr int kActHead = 24;                                    // last_conv

struct ProfEntry {
    int calls = 0;
    double flops = 0, bytes = 0, mfma = 0;      // algorithmic FLOPs / bytes; FLOPs the matrix cores executed
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0;
};

}  // namespace

// which convs of the stack ran in their Winograd form in the last chunk (run_stack_chunk)
struct StackPlan {
    bool wino[8][3] = {};      // [block][conv 1 | 2]
};

struct nhans_ctx {
    int kind = 0, device = 0;
    StackPlan last_plan;
    float* blob_dev = nullptr;
    size_t blob_bytes = 0;
    std::map<std::string, const float*> arr;
    std::map<std::string, size_t> arr_n;
    std::vector<BlockGeo> tower, stack;
    int cond_cols = 0;
    std::vector<int> cond_off;      // column offset of conv j (= 2*block + {0,1})
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0, ws_top = 0;
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
    int lookahead = kCenter;    // option lookahead: frame t of a clip sees the clip end at min(len, t + lookahead + 1) (offline calls)
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

    const float* A(const std::string& n) const {
        auto it = arr.find(n);
        return it == arr.end() ? nullptr : it->second;
    }
    // packed conv weights / per-channel unscale vector of the active precision
    const float* WP(const std::string& n) const { return A(prec ? n + "_h" : n); }
    const float* WS(const std::string& conv) const { return prec ? A(conv + ".ws") : nullptr; }
};

namespace {

int ws_reserve(nhans_ctx* c, size_t bytes) {
    if (bytes <= c->ws_bytes) { c->ws_top = 0; return NHANS_OK; }
    if (c->ws) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->ws), bytes);
    if (e != hipSuccess) {
        char buf[128];
        snprintf(buf, sizeof buf, "workspace hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return fail(NHANS_ENOMEM, buf);
    }
    c->ws_bytes = bytes;
    c->ws_top = 0;
    return NHANS_OK;
}

// Host -> device copy of a small table through the pinned ring, so the caller's (pageable, soon
// destroyed) buffer is never the source of an in-flight asynchronous copy.
int h2d(nhans_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return NHANS_OK;
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (need > c->pin_bytes) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        return NHANS_OK;
    }
    if (c->pin_top + need > c->pin_bytes) {
        HIP_TRY(hipStreamSynchronize(s));
        c->pin_top = 0;
    }
    void* p = c->pin + c->pin_top;
    c->pin_top += need;
    std::memcpy(p, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s));
    return NHANS_OK;
}

template <typename T> T* ws_take(nhans_ctx* c, size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    T* p = reinterpret_cast<T*>(c->ws + c->ws_top);
    c->ws_top += bytes;
    return p;
}
size_t ws_size(size_t count, size_t elem) { return (count * elem + 255) & ~(size_t)255; }

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

void fill_epilogue_defaults(nhans_ctx* c, ConvArgs& a) {
    a.zero = c->A("zero");
    a.sat = c->status_dev;
    a.img_clip = nullptr; a.tf = nullptr; a.tt = nullptr; a.ff = nullptr; a.id_mode = 0; a.id = nullptr; a.id_ld = 0;
    a.idw = nullptr; a.idH = a.idW = 0; a.idsh = a.idsw = 1; a.relu = 1; a.aux = nullptr; a.aux_ld = 0;
    a.cb_stride = 0;
    a.prec = c->prec; a.out_split = c->prec; a.id_split = 0; a.ws = nullptr;
    a.in_scale = a.id_scale = a.out_scale = 1.f;
    a.sat_limit = kSatLimitF16;
    a.variant = c->conv_variant >= 0 ? c->conv_variant : (c->prec == 1 ? 2 : 0);
    a.dbg = kDev ? c->dbg : nullptr;
    a.epi8 = c->epi8;
    a.ilv = c->ilv;
    a.wino = c->wino; a.wino_u = nullptr; a.wino_ws = nullptr;
    a.kscratch = c->kscratch; a.kscratch_bytes = c->kscratch_bytes; a.kcounter = c->kcounter; a.kcounter_n = c->kcounter_n; a.kgroup = 0;
}

ConvSeg make_seg(const float* src, const float* wpk, int H, int W, int C, int KH, int KW, int sh, int sw,
                 bool same) {
    ConvSeg g;
    g.src = src; g.wpk = wpk; g.H = H; g.W = W; g.C = C; g.KH = KH; g.KW = KW; g.sh = sh; g.sw = sw;
    int o, pb;
    if (same) { same_pad(H, KH, sh, &o, &pb); g.pt = pb; same_pad(W, KW, sw, &o, &pb); g.pl = pb; }
    else { g.pt = 0; g.pl = 0; }
    g.nchunks = KH * KW * C / 32;
    return g;
}

void set_out_geometry(ConvArgs& a, int B, int Ho, int Wo, int N, int Nreal, int ldo, float* out) {
    a.Ho = Ho; a.Wo = Wo; a.M = B * Ho * Wo; a.N = N; a.Nreal = Nreal; a.ldo = ldo; a.out = out;
    a.fdHoWo = make_fastdiv((uint32_t)(Ho * Wo));
    a.fdWo = make_fastdiv((uint32_t)Wo);
}

void run_conv(nhans_ctx* c, const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    if (kDev) {      // timing experiment (wrong results): NHANS_ABLATE_TF=1 -> no position table at all
        static const bool no_tf = [] { const char* e = getenv("NHANS_ABLATE_TF"); return e && atoi(e) != 0; }();
        if (no_tf) { a.tf = nullptr; a.tt = nullptr; a.ff = nullptr; }
    }
    if (a.kgroup < 0) {
        // split-K scratch on demand (hipFree / hipMalloc wait for the device: a handful of times per context at most)
        const size_t need = c->split_k ? conv_splitk_scratch_bytes(a) : 0;
        if (need > c->kscratch_bytes && need <= nhans_ctx::kscratch_cap && !c->kscratch_failed) {
            if (c->kscratch) { (void)hipFree(c->kscratch); c->kscratch = nullptr; c->kscratch_bytes = 0; }
            const size_t want = std::min(nhans_ctx::kscratch_cap, std::max(need, (size_t)32 << 20));
            if (hipMalloc(reinterpret_cast<void**>(&c->kscratch), want) == hipSuccess) c->kscratch_bytes = want;
            else { (void)hipGetLastError(); c->kscratch = nullptr; c->kscratch_failed = true; }
        }
        a.kscratch = c->split_k ? c->kscratch : nullptr;
        a.kscratch_bytes = c->kscratch_bytes;
    }
    // profiled under the name of the kernel variant that ran (the variant is chosen per layer)
    Prof p(c, s, nullptr);
    const char* name = "conv_igemm";
    double mfma = 0;
    double fl = launch_conv_igemm(a, s, &name, &mfma);
    p.done(fl, 0, name, mfma);
}

// Which convs of the stack run in their Winograd form (conv_wino.hip), for one chunk of frame windows.  NOT a restatement
// of the kernel's conditions: run_stack_chunk() builds every launch's ConvArgs twice -- a planning pass that asks
// conv_wino_eligible() about those very arguments, then the launching pass that takes layouts and saturation limits
// from the answers (round-4 advisor finding: a second predicate that left out the 32-bit offset bound, aux, kgroup ...
// could disagree with the kernel, and the producer would already have written the other layout).
bool wino_form(const ConvArgs& a) { return a.variant >= 2 && a.kgroup >= 0 && conv_wino_eligible(a); }
float sat_limit_for(const StackPlan& p, int b, int cv) { return b >= 0 && b < 8 && p.wino[b][cv] ? kSatLimitWinoInput : kSatLimitF16; }

// Is stack tensor (block b; cv 0: conv1's output, 1: the block's output) stored as f32 NHWC in the split-f16 mode?  Yes if
// every launch that reads it is a Winograd launch -- conv_wino.hip reads either layout (its transform works in f32 and
// re-splits: with an f32 input it has no hi + lo to add up, 64 of its ~215 instructions per chunk), the direct kernels
// stage split pieces straight into MFMA operands -- and the launch that writes it is direct_conv64 or a Winograd launch.
// The values are the same scaled, clamped ones a split store would hold to 22 bits; 4 bytes per element either way.
// (wino_f32 == 2, a test value: f32 whatever the readers are -- launch_conv_igemm() must then refuse the reader.
//  wino_f32 == 3, a test value: ONLY the output of resblock1_2 is f32 -- its conv2 then has a split residual and an f32
//  output, the one layout pair conv_wino's epilogue does not implement: launch_conv_wino() must refuse it.)
bool stored_f32(const nhans_ctx* c, const StackPlan& p, int b, int cv) {
    if (c->prec != 1 || !c->wino_f32 || b < 0 || b > 7) return false;
    if (c->wino_f32 == 2) return b < 4 && !(b == 3 && cv == 1);
    if (c->wino_f32 == 3) return b == 1 && cv == 1;
    if (cv == 0) return p.wino[b][2] && (b == 0 || p.wino[b][1]);
    if (b == 7) return false;
    const BlockGeo& nx = c->stack[b + 1];             // read by conv1 of the next block and, in an identity block, by its conv2's epilogue
    return p.wino[b][2] && p.wino[b + 1][1] && nx.cin == nx.cout && p.wino[b + 1][2];
}

// Tap on the finished tensor `idx` (`words` values of `chan` channels, stored in the active precision's layout).
// Calibration: its running |x| maximum.  Debug capture: the tensor itself as f32 NHWC, out of its layout and exponent
// (the chunks of a call follow one another in cap_out).
void tap(nhans_ctx* c, int idx, const float* buf, size_t words, int chan, hipStream_t s, bool f32_layout = false) {
    if (c->calibrating) launch_absmax(buf, words, c->prec && !f32_layout, c->up(idx), c->amax_dev + idx, s);
    if (c->cap_idx != idx) return;
    if (!c->prec) note_launch("activation tap copy", hipMemcpyAsync(c->cap_out, buf, words * 4, hipMemcpyDeviceToDevice, s));
    else if (f32_layout) launch_scale_copy(buf, words, c->up(idx), c->cap_out, s);
    else launch_unsplit(buf, (int64_t)(words / chan), chan, c->up(idx), c->cap_out, s);
    c->cap_out += words;
}

// ---- embedding tower for `n` context images already in HBM ----------------------------------
int embed_impl(nhans_ctx* c, const float* ctx_lm, int n, float* emb_out, float* X, float* Ab, float* Y,
               hipStream_t s) {
    const auto& T = c->tower;
    for (int i0 = 0; i0 < n; i0 += c->contexts_per_chunk) {
        const int nc = std::min(c->contexts_per_chunk, n - i0);
        const float* img = ctx_lm + (size_t)i0 * kCtxFrames * kBins;
        float *x = X, *a1 = Ab, *y = Y;
        for (int b = 0; b < 4; ++b) {
            const BlockGeo& g = T[b];
            const std::string p = "t" + std::to_string(b);
            if (b == 0) {
                DirectArgs d{};
                d.src = img; d.w = c->A(p + ".c1.w"); d.H = g.hin; d.W = g.win; d.KH = g.kh; d.KW = g.kw;
                d.sh = g.sh; d.sw = g.sw;
                int o; same_pad(g.hin, g.kh, g.sh, &o, &d.pt); same_pad(g.win, g.kw, g.sw, &o, &d.pl);
                d.Ho = g.hout; d.Wo = g.wout; d.M = nc * g.hout * g.wout; d.out = a1;
                d.cb = c->A(p + ".c1.cb"); d.cb_stride = 0; d.img_clip = nullptr; d.tf = nullptr; d.tt = nullptr; d.ff = nullptr;
                d.relu = 1; d.fdHoWo = make_fastdiv(g.hout * g.wout); d.fdWo = make_fastdiv(g.wout);
                d.out_split = c->prec; d.sat = c->prec ? c->status_dev : nullptr; d.out_scale = c->down(TA(0, 0)); d.sat_limit = kSatLimitF16;
                Prof pr(c, s, "direct_conv64");
                launch_direct_conv64(d, s);
                pr.done(2.0 * d.M * g.kh * g.kw * 64, 0);
            } else {
                ConvArgs a{};
                fill_epilogue_defaults(c, a);
                a.nseg = 1;
                a.seg[0] = make_seg(x, c->WP(p + ".c1.wpk"), g.hin, g.win, g.cin, g.kh, g.kw, g.sh, g.sw, true);
                set_out_geometry(a, nc, g.hout, g.wout, g.cout, g.cout, g.cout, a1);
                a.cb = c->A(p + ".c1.cb");
                a.ws = c->WS(p + ".c1");
                a.in_scale = c->up(TA(b - 1, 1)); a.out_scale = c->down(TA(b, 0));
                a.kgroup = -1;                  // a handful of context images: grouped sum, split-K when small
                run_conv(c, a, s);
            }
            tap(c, TA(b, 0), a1, (size_t)nc * g.hout * g.wout * g.cout, g.cout, s);
            ConvArgs a{};
            fill_epilogue_defaults(c, a);
            a.nseg = 1;
            a.seg[0] = make_seg(a1, c->WP(p + ".c2.wpk"), g.hout, g.wout, g.cout, g.kh, g.kw, 1, 1, true);
            if (b == 0) {
                a.id_mode = 2; a.id = img; a.idH = g.hin; a.idW = g.win; a.idsh = g.sh; a.idsw = g.sw;
                a.idw = c->A(p + ".c2.idw");
            } else {
                a.nseg = 2;
                a.seg[1] = make_seg(x, c->WP(p + ".c2.wpk_t"), g.hin, g.win, g.cin, 1, 1, g.sh, g.sw, false);
            }
            set_out_geometry(a, nc, g.hout, g.wout, g.cout, g.cout, g.cout, y);
            a.cb = c->A(p + ".c2.cb");
            a.ws = c->WS(p + ".c2");
            // (the `_transform` segment reads x, whose exponent tie_exponents() keeps equal to a1's: one accumulator)
            a.in_scale = c->up(TA(b, 0)); a.out_scale = c->down(TA(b, 1));
            run_conv(c, a, s);                  // (stride 1: halo kernel; measured faster than split-K here)
            tap(c, TA(b, 1), y, (size_t)nc * g.hout * g.wout * g.cout, g.cout, s);
            std::swap(x, y);
        }
        const BlockGeo& g = T[3];
        Prof pr(c, s, "avgpool");
        launch_avgpool(x, nc, g.hout * g.wout, g.cout, c->prec, c->up(TA(3, 1)), emb_out + (size_t)i0 * kEmb, s);
        pr.done(0, (double)nc * g.hout * g.wout * g.cout * 4);
    }
    return NHANS_OK;
}

size_t tower_buf_floats(const nhans_ctx* c) {
    size_t m = 0;
    for (const auto& g : c->tower) m = std::max(m, (size_t)g.hout * g.wout * g.cout);
    return m * (size_t)c->contexts_per_chunk;
}
size_t stack_buf_floats(const nhans_ctx* c, int64_t wf) {
    size_t m = 0;
    for (const auto& g : c->stack) m = std::max(m, (size_t)g.hout * g.wout * g.cout);
    return m * (size_t)wf;
}

// ---- conditioned stack + head ---------------------------------------------------------------
struct StackBufs {
    int* f_clip; int* f_t; int* f_T; int64_t* foff_dev; float* cb_all;
    float* X; float* A; float* Y;
    float* T;       // f32 output of a block's 1x1 `_transform` conv when its conv2 runs in Winograd form
};

// floats per frame window of StackBufs::T: the largest conv2 output among the channel-changing blocks whose conv2
// has a Winograd form (4x4 filters: resblock2_1)
size_t transform_buf_floats(const nhans_ctx* c, int64_t wf) {
    size_t m = 0;
    for (const auto& g : c->stack)
        if (g.cin != g.cout && g.cin > 1 && g.kh == 4) m = std::max(m, (size_t)g.hout * g.wout * g.cout);
    return m * (size_t)wf;
}

size_t stack_ws_bytes(const nhans_ctx* c, int64_t total, int nclips, int64_t wf) {
    size_t b = 3 * ws_size(total, 4) + ws_size(nclips + 1, 8) + ws_size((size_t)nclips * c->cond_cols, 4);
    b += 3 * ws_size(stack_buf_floats(c, wf), 4);
    b += ws_size(transform_buf_floats(c, wf), 4);
    return b;
}

void stack_take(nhans_ctx* c, int64_t total, int nclips, int64_t wf, StackBufs* sb) {
    sb->f_clip = ws_take<int>(c, total); sb->f_t = ws_take<int>(c, total); sb->f_T = ws_take<int>(c, total);
    sb->foff_dev = ws_take<int64_t>(c, nclips + 1);
    sb->cb_all = ws_take<float>(c, (size_t)nclips * c->cond_cols);
    const size_t nb = stack_buf_floats(c, wf);
    sb->X = ws_take<float>(c, nb); sb->A = ws_take<float>(c, nb); sb->Y = ws_take<float>(c, nb);
    sb->T = ws_take<float>(c, transform_buf_floats(c, wf));
}

// Runs blocks [0, upto) for frames [g0, g0+n); returns the buffer holding the last output.
// upto = 8: whole stack; upto = 9: + last_conv (output in sb.A).
// Two passes over the same code: pass 0 builds every conv's arguments and records which of them the Winograd kernel
// accepts (StackPlan), pass 1 builds them again with the tensor layouts and saturation limits that follow from the plan
// and launches.  A launch whose eligibility differs between the passes is an error, not a fallback.
// rb (nullable): per-frame first window row in `logmag` (online enhancement, WinRows::rb); null: frame g's window starts at
// row g - 17
float* run_stack_chunk(nhans_ctx* c, const float* logmag, const int* rb, const StackBufs& sb, int64_t g0, int n, int upto,
                       hipStream_t s) {
    StackPlan plan;
    float* result = nullptr;
    const int* clipmap = sb.f_clip + g0;
    for (int pass = 0; pass < 2; ++pass) {
    const bool go = pass == 1;
    // (pass 0: record; pass 1: the launch must be the one that was planned)
    // (a launch that failed or was refused ends the chunk: nothing later may run on a buffer that was never written)
    auto dead = [&] { return go && launch_error_pending(); };
    auto conv = [&](int b, int cv, const ConvArgs& a) {
        const bool w = wino_form(a);
        if (!go) { plan.wino[b][cv] = w; return; }
        if (dead()) return;
        if (w != plan.wino[b][cv]) {
            note_refusal("stack conv whose Winograd eligibility changed between planning and launch");
            return;
        }
        run_conv(c, a, s);
    };
    // frame b's 35 x 201 image = rows g0 + b - 17 ... of the log-magnitude spectrogram, zero rows outside its clip
    // (SN/apply.py:170-186,378: strided_crop, never materialised -- the first conv and the 1 -> 64 residual of
    // resblock1_1 read the spectrogram where it lies)
    // (rows are counted from the chunk's first frame -- the tensor pointer handed to the kernels is logmag + g0 * 201 --, so the
    // kernels' 32-bit element indices stay below (frames_per_chunk + 35) * 201 however long the batch is)
    // (online: rows are where the per-frame table rb says, in a tensor small enough for 32-bit indices, WinRows::rb)
    const WinRows win{sb.f_t + g0, sb.f_T + g0, -kCenter, kCenter, rb ? rb + g0 : nullptr};
    const float* const lm_chunk = rb ? logmag : logmag + (size_t)g0 * kBins;
    float *x = sb.X, *a1 = sb.A, *y = sb.Y;
    // pass 0 plans the WHOLE stack whatever `upto` is -- the layout of block b's output follows from block b + 1's
    // readers, and the debug entry point (upto = block + 1) must see the tensors the production call writes
    for (int b = 0; b < 8 && (b < upto || !go); ++b) {
        const BlockGeo& g = c->stack[b];
        const std::string p = "m" + std::to_string(b);
        const float* cb1 = sb.cb_all + c->cond_off[2 * b];
        const float* cb2 = sb.cb_all + c->cond_off[2 * b + 1];
        if (b == 0) {
            DirectArgs d{};
            d.src = lm_chunk; d.win = win; d.w = c->A(p + ".c1.w"); d.H = g.hin; d.W = g.win; d.KH = g.kh; d.KW = g.kw;
            d.sh = 1; d.sw = 1;
            int o; same_pad(g.hin, g.kh, 1, &o, &d.pt); same_pad(g.win, g.kw, 1, &o, &d.pl);
            d.Ho = g.hout; d.Wo = g.wout; d.M = n * g.hout * g.wout; d.out = a1;
            d.cb = cb1; d.cb_stride = c->cond_cols; d.img_clip = clipmap;
            d.tf = c->A(p + ".c1.tf"); d.tt = c->A(p + ".c1.tt"); d.ff = c->A(p + ".c1.ff");
            if (!d.tt || !d.ff) d.tt = d.ff = nullptr;
            d.relu = 1; d.out_split = c->prec && !stored_f32(c, plan, 0, 0); d.sat = c->prec ? c->status_dev : nullptr;
            d.out_scale = c->down(SA(0, 0)); d.sat_limit = sat_limit_for(plan, 0, 2);
            d.fdHoWo = make_fastdiv(g.hout * g.wout); d.fdWo = make_fastdiv(g.wout);
            if (go && !dead()) {
                Prof pr(c, s, "direct_conv64");
                launch_direct_conv64(d, s);
                pr.done(2.0 * d.M * g.kh * g.kw * 64, 0);
            }
        } else {
            ConvArgs a{};
            fill_epilogue_defaults(c, a);
            a.nseg = 1;
            a.seg[0] = make_seg(x, c->WP(p + ".c1.wpk"), g.hin, g.win, g.cin, g.kh, g.kw, g.sh, g.sw, true);
            set_out_geometry(a, n, g.hout, g.wout, g.cout, g.cout, g.cout, a1);
            a.cb = cb1; a.cb_stride = c->cond_cols; a.img_clip = clipmap;
            a.tf = c->A(p + ".c1.tf"); a.tt = c->A(p + ".c1.tt"); a.ff = c->A(p + ".c1.ff");
            a.ws = c->WS(p + ".c1");
            a.wino_u = c->A(p + ".c1.wino"); a.wino_ws = c->A(p + ".c1.wino.ws");
            a.in_scale = c->up(SA(b - 1, 1)); a.out_scale = c->down(SA(b, 0));
            a.sat_limit = sat_limit_for(plan, b, 2);
            a.in_f32 = stored_f32(c, plan, b - 1, 1); a.out_split = c->prec && !stored_f32(c, plan, b, 0);
            conv(b, 1, a);
        }
        if (go) tap(c, SA(b, 0), a1, (size_t)n * g.hout * g.wout * g.cout, g.cout, s, stored_f32(c, plan, b, 0));
        ConvArgs a{};
        fill_epilogue_defaults(c, a);
        a.nseg = 1;
        a.seg[0] = make_seg(a1, c->WP(p + ".c2.wpk"), g.hout, g.wout, g.cout, g.kh, g.kw, 1, 1, true);
        a.cb = cb2; a.cb_stride = c->cond_cols; a.img_clip = clipmap;
        a.tf = c->A(p + ".c2.tf"); a.tt = c->A(p + ".c2.tt"); a.ff = c->A(p + ".c2.ff");
        a.idw = c->A(p + ".c2.idw");
        a.ws = c->WS(p + ".c2");
        a.wino_u = c->A(p + ".c2.wino"); a.wino_ws = c->A(p + ".c2.wino.ws");
        a.in_scale = c->up(SA(b, 0)); a.out_scale = c->down(SA(b, 1));
        a.sat_limit = sat_limit_for(plan, b + 1, 1);
        a.in_f32 = stored_f32(c, plan, b, 0); a.out_split = c->prec && !stored_f32(c, plan, b, 1);
        float* out;
        if (b == 0) {                       // 1 -> 64 transform on the window image itself
            a.id_mode = 2; a.id = lm_chunk; a.id_win = win; a.idH = g.hin; a.idW = g.win; a.idsh = 1; a.idsw = 1;
            out = x;
        } else if (g.cin == g.cout) {       // identity shortcut, written in place over the block input
            a.id_mode = 1; a.id = x; a.id_ld = g.cout; a.id_split = c->prec && !stored_f32(c, plan, b - 1, 1);
            a.id_scale = c->up(SA(b - 1, 1));
            // (in place only if input and output share a layout: a thread's output bytes are its residual bytes then)
            out = stored_f32(c, plan, b - 1, 1) == stored_f32(c, plan, b, 1) ? x : y;
        } else {
            // Channel-changing block.  If its conv2 -- as a one-segment conv with an f32 residual tensor -- has a
            // Winograd form, the 1x1 strided `_transform` conv (which cannot ride in the K loop of the transformed
            // domain; 3 % of the block's MACs) runs first on its own into an f32 tensor that conv2's epilogue then adds
            // like a residual (the bias of both is in conv2's bias row).  Otherwise it is extra K columns of conv2.
            ConvArgs w = a;
            w.id_mode = 1; w.id = sb.T; w.id_ld = g.cout; w.id_split = 0;
            w.idw = c->A("head.dense.idw");     // ones
            set_out_geometry(w, n, g.hout, g.wout, g.cout, g.cout, g.cout, y);
            if (go ? plan.wino[b][2] : wino_form(w)) {
                ConvArgs t{};
                fill_epilogue_defaults(c, t);
                t.nseg = 1;
                t.seg[0] = make_seg(x, c->WP(p + ".c2.wpk_t"), g.hin, g.win, g.cin, 1, 1, g.sh, g.sw, false);
                set_out_geometry(t, n, g.hout, g.wout, g.cout, g.cout, g.cout, sb.T);
                t.cb = c->A("zero"); t.cb_stride = 0;
                t.ws = c->WS(p + ".c2");            // (conv2 and the transform share one column scale: fold.py emit())
                t.relu = 0; t.out_split = 0;
                t.in_scale = c->up(SA(b - 1, 1));   // (f32 output: no exponent)
                if (go && !dead()) {
                    if (c->stream_1x1 && conv_1x1_stream_eligible(t)) {       // 1.75 GB in, 3.5 GB out, 16 KFLOP per output pixel: a stream
                        Prof pr(c, s, "conv_1x1_stream");
                        launch_conv_1x1_stream(t, s);
                        const double fl = 2.0 * (double)t.M * g.cin * g.cout;
                        pr.done(fl, (double)t.M * (g.cin + g.cout) * 4.0, nullptr, 3.0 * fl);
                    } else {
                        run_conv(c, t, s);
                    }
                }
                a = w;
            } else {                        // (x and a1 share one exponent)
                a.nseg = 2;
                a.seg[1] = make_seg(x, c->WP(p + ".c2.wpk_t"), g.hin, g.win, g.cin, 1, 1, g.sh, g.sw, false);
            }
            out = y;
        }
        set_out_geometry(a, n, g.hout, g.wout, g.cout, g.cout, g.cout, out);
        conv(b, 2, a);
        if (go) tap(c, SA(b, 1), out, (size_t)n * g.hout * g.wout * g.cout, g.cout, s, stored_f32(c, plan, b, 1));
        if (out == y) std::swap(x, y);
    }
    result = x;
    if (upto >= 9 && go && !dead()) {       // last_conv [5,1] VALID + BN + ReLU  (SN/main.py:232-236)
        const BlockGeo& g = c->stack[7];
        ConvArgs a{};
        fill_epilogue_defaults(c, a);
        a.nseg = 1;
        a.seg[0] = make_seg(x, c->WP("head.conv.wpk"), g.hout, g.wout, g.cout, g.hout, 1, 1, 1, false);
        set_out_geometry(a, n, 1, g.wout, 512, 512, 512, a1);
        a.cb = c->A("head.conv.cb");
        a.ws = c->WS("head.conv");
        a.in_scale = c->up(SA(7, 1)); a.out_scale = c->down(kActHead);
        run_conv(c, a, s);
        tap(c, kActHead, a1, (size_t)n * g.wout * 512, 512, s);
        result = a1;
    }
    }
    c->last_plan = plan;
    return result;
}

// The stack + head over `total` frame windows whose per-frame tables (sb.f_clip, f_t, f_T) are in place.  win_src / rb:
// the window source (rb nullable, see run_stack_chunk); centre [total, 201]: the frames' own rows, the head's identity
// term (mixed_central, SN/main.py:242) -- offline that is win_src itself.
int mask_net_run(nhans_ctx* c, const float* win_src, const int* rb, const float* centre, int64_t total, int nclips,
                 const float* ea, const float* eb, float* logits, float* denoised, const StackBufs& sb, int64_t wf,
                 hipStream_t s) {
    {
        Prof pr(c, s, "cond_proj");
        launch_cond(ea, eb, nclips, c->A("cond.w"), c->A("cond.base"), c->cond_cols, sb.cb_all, s);
        pr.done(2.0 * nclips * 2 * kEmb * c->cond_cols, 0);
    }
    const BlockGeo& g = c->stack[7];
    for (int64_t g0 = 0; g0 < total; g0 += wf) {
        const int n = (int)std::min<int64_t>(wf, total - g0);
        float* hc = run_stack_chunk(c, win_src, rb, sb, g0, n, 9, s);
        if (launch_error_pending()) break;      // (reported by the entry point: NHANS_EHIP naming the launch)
        // last_dense 13312 -> 201 (+bias) and denoised = mixed_central + out  (SN/main.py:237-242)
        ConvArgs a{};
        fill_epilogue_defaults(c, a);
        a.nseg = 1;
        a.seg[0] = make_seg(hc, c->WP("head.dense.wpk"), 1, 1, g.wout * 512, 1, 1, 1, 1, false);
        set_out_geometry(a, n, 1, 1, 256, kBins, kBins, denoised + g0 * kBins);
        a.cb = c->A("head.dense.cb");
        a.ws = c->WS("head.dense");
        a.out_split = 0;
        a.relu = 0;
        a.in_scale = c->up(kActHead);
        a.id_mode = 1; a.id = centre + g0 * kBins; a.id_ld = kBins; a.idw = c->A("head.dense.idw");
        if (logits) { a.aux = logits + g0 * kBins; a.aux_ld = kBins; }
        a.kgroup = -1;                          // K = 13312 over a few hundred frames: grouped sum, split-K when small
        run_conv(c, a, s);
    }
    return NHANS_OK;
}

int mask_net_impl(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                  const float* eb, float* logits, float* denoised, const StackBufs& sb, int64_t wf,
                  hipStream_t s) {
    const int64_t total = foff[nclips];
    { int rc = h2d(c, sb.foff_dev, foff, (nclips + 1) * sizeof(int64_t), s); if (rc) return rc; }
    launch_frame_index(sb.foff_dev, nclips, total, c->lookahead, sb.f_clip, sb.f_t, sb.f_T, s);
    return mask_net_run(c, logmag, nullptr, logmag, total, nclips, ea, eb, logits, denoised, sb, wf, s);
}

// ---- STFT / iSTFT host-side block tables ----------------------------------------------------
struct HostTables {
    std::vector<int64_t> soff, foff, ooff;
    std::vector<int> bclip, bpos;
};

int stft_impl(nhans_ctx* c, const float* wav, const int64_t* soff, int nclips, int maxf, float* logmag,
              float* phase, int64_t* dev_tables /*3*(nclips+1)*/, int* dev_blocks, std::vector<int64_t>* foff_out,
              hipStream_t s, const char* prof_name = nullptr) {
    std::vector<int64_t> foff(nclips + 1, 0);
    std::vector<int> bclip, bf0;
    for (int i = 0; i < nclips; ++i) {
        int64_t t = nhans_num_frames(soff[i + 1] - soff[i]);
        if (t > kMaxFramesPerClip) return fail(NHANS_EINVAL, "clip " + std::to_string(i) + " has more than " +
                                               std::to_string(kMaxFramesPerClip) + " frames (32-bit offsets within a clip)");
        if (maxf > 0) {
            if (t < maxf) return fail(NHANS_ESHORT, "conditioning clip " + std::to_string(i) + " has " +
                                      std::to_string(t) + " frames; " + std::to_string(maxf) + " needed");
            t = maxf;
        }
        foff[i + 1] = foff[i] + t;
        for (int f0 = 0; f0 < t; f0 += kStftFramesPerBlock) { bclip.push_back(i); bf0.push_back(f0); }
    }
    const int nb = (int)bclip.size();
    int rc = h2d(c, dev_tables, soff, (nclips + 1) * 8, s); if (rc) return rc;
    rc = h2d(c, dev_tables + (nclips + 1), foff.data(), (nclips + 1) * 8, s); if (rc) return rc;
    rc = h2d(c, dev_blocks, bclip.data(), (size_t)nb * 4, s); if (rc) return rc;
    rc = h2d(c, dev_blocks + nb, bf0.data(), (size_t)nb * 4, s); if (rc) return rc;
    ClipTable t{dev_tables, dev_tables + (nclips + 1), nullptr};
    Prof pr(c, s, prof_name ? prof_name : phase ? "stft_features" : "stft_context_features");   // (contexts: log-magnitude only, 200 frames per clip)
    launch_stft(wav, t, dev_blocks, dev_blocks + nb, nb, c->A("tw400"), c->A("window"), logmag, phase, s);
    pr.done(0, (double)foff[nclips] * (kHop * 4 + (phase ? 2 : 1) * kBins * 4));
    if (foff_out) *foff_out = foff;
    return NHANS_OK;
}

size_t stft_blocks(const int64_t* soff, int nclips, int maxf) {
    size_t nb = 0;
    for (int i = 0; i < nclips; ++i) {
        int64_t t = nhans_num_frames(soff[i + 1] - soff[i]);
        if (maxf > 0 && t > maxf) t = maxf;
        nb += (size_t)((t + kStftFramesPerBlock - 1) / kStftFramesPerBlock);
    }
    return nb;
}

int istft_impl(nhans_ctx* c, const float* logmag, const float* phase, const int64_t* foff, int nclips,
               const int64_t* ooff, float* wav_out, int64_t* dev_tables, int* dev_blocks, hipStream_t s,
               const char* prof_name = "istft_ola") {
    std::vector<int> bclip, bh0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t t = foff[i + 1] - foff[i];
        if (t > kMaxFramesPerClip) return fail(NHANS_EINVAL, "clip " + std::to_string(i) + " has more than " +
                                               std::to_string(kMaxFramesPerClip) + " frames (32-bit offsets within a clip)");
        if (t <= 0) continue;
        for (int h0 = 0; h0 < t + 2; h0 += kIstftHopsPerBlock) { bclip.push_back(i); bh0.push_back(h0); }
    }
    const int nb = (int)bclip.size();
    int rc = h2d(c, dev_tables, foff, (nclips + 1) * 8, s); if (rc) return rc;
    rc = h2d(c, dev_tables + (nclips + 1), ooff, (nclips + 1) * 8, s); if (rc) return rc;
    rc = h2d(c, dev_blocks, bclip.data(), (size_t)nb * 4, s); if (rc) return rc;
    rc = h2d(c, dev_blocks + nb, bh0.data(), (size_t)nb * 4, s); if (rc) return rc;
    ClipTable t{nullptr, dev_tables, dev_tables + (nclips + 1)};
    Prof pr(c, s, prof_name);
    launch_istft(logmag, phase, t, dev_blocks, dev_blocks + nb, nb, c->A("tw400"), c->A("wsyn"), wav_out, s);
    pr.done(0, (double)foff[nclips] * (kHop * 4 + 2 * kBins * 4));
    return NHANS_OK;
}

size_t istft_blocks(const int64_t* foff, int nclips) {
    size_t nb = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t t = foff[i + 1] - foff[i];
        if (t > 0) nb += (size_t)((t + 2 + kIstftHopsPerBlock - 1) / kIstftHopsPerBlock);
    }
    return nb;
}

// Two tensors that feed ONE accumulator (a channel-changing block's conv2 reads its conv1 output and, through the
// `_transform` segment, the block input) must carry one exponent: the larger of the two.
void tie_exponents(nhans_ctx* c) {
    auto tie = [&](int i, int j) { c->act_exp[i] = c->act_exp[j] = std::max(c->act_exp[i], c->act_exp[j]); };
    for (int b = 1; b < 4; ++b) tie(TA(b - 1, 1), TA(b, 0));
    for (int b = 1; b < 8; ++b)
        if (c->stack[b].cin != c->stack[b].cout) tie(SA(b - 1, 1), SA(b, 0));
}

// End of a calibration bracket: maxima -> exponents (merge: only raise).
int finish_calibration(nhans_ctx* c, bool merge) {
    c->calibrating = false;
    unsigned bits[kNumAct];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bits, c->amax_dev, sizeof bits, hipMemcpyDeviceToHost));
    int e_new[kNumAct];
    for (int i = 0; i < kNumAct; ++i) {
        float m;
        std::memcpy(&m, &bits[i], 4);
        if (!std::isfinite(m)) {
            // merge (the bracket round a saturated batch's f32 rerun): an input that is NaN / Inf itself makes every
            // maximum non-finite -- that says nothing about the range, the exponent stays; a calibration proper refuses
            if (!merge) return fail(NHANS_EINVAL, "calibration: tensor " + std::to_string(i) + " reached a non-finite value");
            e_new[i] = c->act_exp[i];
            continue;
        }
        c->act_amax[i] = m;
        int k = 0;
        if (m > 0.f) (void)frexpf(m, &k);               // m = f * 2^k, f in [0.5, 1)  =>  m * 2^-(k - T) <= 2^T
        // (a tensor the pass never wrote -- or a pass that failed before its first launch -- keeps its exponent)
        e_new[i] = m > 0.f ? k - kActTargetLog2 : c->act_exp[i];
    }
    for (int i = 0; i < kNumAct; ++i) c->act_exp[i] = merge ? std::max(c->act_exp[i], e_new[i]) : e_new[i];
    tie_exponents(c);
    return NHANS_OK;
}

int check_ctx(nhans_ctx* c) {
    if (!c) return fail(NHANS_EINVAL, "null context");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(NHANS_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return NHANS_OK;
}

// A launch the runtime rejected anywhere in the sequence just issued -> NHANS_EHIP.
int launch_status() {
    const char* where = "";
    const hipError_t e = take_launch_error(&where);
    if (e == hipSuccess) return NHANS_OK;
    return fail(NHANS_EHIP, std::string("kernel launch failed: ") + where + ": " + hipGetErrorString(e));
}

// Bracket of one hot-path entry point: selects the device, orders the call behind the previous
// call on this context when that one ran on another stream (they share workspace, pinned tables
// and split-K tickets), and on the way out collects launch failures and marks the new tail.
struct Call {
    nhans_ctx* c;
    hipStream_t s;
    int rc;
    Call(nhans_ctx* c_, void* stream) : c(c_), s(static_cast<hipStream_t>(stream)), rc(check_ctx(c_)) {
        if (rc) return;
        (void)take_launch_error(nullptr);               // (a stale record of another context's failure)
        // (The runtime's sticky per-thread "last error" may hold something an earlier HIP call of the APPLICATION left
        // there -- hipErrorPeerAccessAlreadyEnabled, an invalid-value from a pointer-attribute probe: it is not read
        // here, neither blamed on this library's kernels nor cleared on the application's behalf; launches are checked
        // by their own return code, NHANS_LAUNCH.  Round 3 refused to run on top of it; the advisor was right that a
        // benign leftover then disabled the whole library.)
        if (c->have_tail && c->last_stream != s) {
            const hipError_t e = hipStreamWaitEvent(s, c->tail_ev, 0);
            if (e != hipSuccess) rc = fail(NHANS_EHIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
        }
    }
    int finish(int body_rc) {
        const int lrc = launch_status();
        if (hipEventRecord(c->tail_ev, s) == hipSuccess) { c->have_tail = true; c->last_stream = s; }
        return body_rc ? body_rc : lrc;
    }
};

__global__ void launch_probe_kernel(int* out) {
    extern __shared__ int probe_lds[];
    probe_lds[threadIdx.x] = threadIdx.x;
    __syncthreads();
    if (out && threadIdx.x == 0) *out = probe_lds[63];
}

}  // namespace

// ================================================================================================
extern "C" {

int nhans_abi_version(void) { return NHANS_ABI_VERSION; }
const char* nhans_last_error(void) { return g_err.c_str(); }

int64_t nhans_num_frames(int64_t n) { return n < kWin ? 0 : 1 + (n - kWin) / kHop; }

static int enhance_clips_body(nhans_ctx* c, const float* mix, const int64_t* moff, int nclips, const float* ca,
                              const int64_t* caoff, const float* cbw, const int64_t* cboff, float* den_wav,
                              float* mixed_wav, float* logmag_out, float* phase_out, float* logits_out, float* emb_out,
                              void* stream);

// Activation exponents of a fresh context: one pass of the whole path at precision 0 over a built-in batch of two clips
// -- a two-second mixture of a gliding harmonic voice with syllabic amplitude modulation and noise, conditioned once on
// two noise recordings and once on (silence, noise): an all-zero recording is the reference's default `--pos` and
// drives the tower with the constant silence floor -- with every tensor's maximum recorded.  Deterministic (LCG).
static int calibrate_builtin(nhans_ctx* c) {
    const int64_t n_mix = kWin + (int64_t)kHop * 197, n_ctx = kWin + (int64_t)kHop * (kCtxFrames - 1);
    std::vector<float> mix(2 * n_mix), ca(2 * n_ctx), cb(2 * n_ctx);
    uint32_t lcg = 0x2545F491u;
    auto noise = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(int32_t)lcg * (1.0f / 2147483648.0f); };
    double ph = 0.0;
    for (int64_t i = 0; i < n_mix; ++i) {
        const double t = (double)i / 16000.0;
        ph += 2.0 * M_PI * (110.0 + 35.0 * t) / 16000.0;
        double v = 0.0;
        for (int h = 1; h <= 12; ++h) v += std::sin(h * ph) / h;
        const double am = 0.5 - 0.5 * std::cos(2.0 * M_PI * 4.0 * t);
        mix[i] = (float)(0.22 * am * v) + 0.05f * noise();
        mix[n_mix + i] = 0.35f * mix[i] + 0.12f * noise();
    }
    float lp = 0.f;
    for (int64_t i = 0; i < n_ctx; ++i) {
        lp = 0.9f * lp + 0.1f * noise();
        ca[i] = 0.6f * lp;                    // clip 0: low-passed noise / white noise
        cb[i] = 0.1f * noise();
        ca[n_ctx + i] = 0.f;                  // clip 1: silence / white noise
        cb[n_ctx + i] = 0.25f * noise();
    }
    const int64_t moff[3] = {0, n_mix, 2 * n_mix}, coff[3] = {0, n_ctx, 2 * n_ctx};
    float* dev = nullptr;
    const size_t words = (size_t)4 * n_mix + (size_t)4 * n_ctx;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dev), words * 4));
    float *d_mix = dev, *d_den = dev + 2 * n_mix, *d_ca = dev + 4 * n_mix, *d_cb = d_ca + 2 * n_ctx;
    hipError_t e = hipMemcpy(d_mix, mix.data(), mix.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_ca, ca.data(), ca.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cb, cb.data(), cb.size() * 4, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? NHANS_OK : fail(NHANS_EHIP, std::string("calibration upload: ") + hipGetErrorString(e));
    if (!rc) {
        const int prec = c->prec;
        c->prec = 0;
        c->calibrating = true;
        (void)take_launch_error(nullptr);
        rc = enhance_clips_body(c, d_mix, moff, 2, d_ca, coff, d_cb, coff, d_den, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr);
        if (!rc) rc = launch_status();
        const int frc = finish_calibration(c, false);       // (synchronises)
        if (!rc) rc = frc;
        c->prec = prec;
    }
    (void)hipFree(dev);
    return rc;
}

int nhans_create(int model_kind, const void* blob, size_t nbytes, int device_id, nhans_ctx** out) {
    return nhans_create_ex(model_kind, blob, nbytes, device_id, nullptr, 0, out);
}

int nhans_create_ex(int model_kind, const void* blob, size_t nbytes, int device_id, const int* act_exp, int n_exp,
                    nhans_ctx** out) {
    if (!out || !blob) return fail(NHANS_EINVAL, "null argument");
    *out = nullptr;
    if (act_exp) {
        if (n_exp != kNumAct) return fail(NHANS_EINVAL, "activation exponents: need NHANS_NUM_ACTIVATIONS values");
        for (int i = 0; i < n_exp; ++i)
            if (act_exp[i] < -60 || act_exp[i] > 60) return fail(NHANS_EINVAL, "activation exponent outside [-60, 60]");
    }
    if (model_kind != NHANS_DENOISER && model_kind != NHANS_SEPARATOR) return fail(NHANS_EINVAL, "bad model_kind");
    if (nbytes < sizeof(BlobHeader)) return fail(NHANS_EINVAL, "blob too short");
    const BlobHeader* h = static_cast<const BlobHeader*>(blob);
    if (std::memcmp(h->magic, "NHANSFW1", 8) != 0) return fail(NHANS_EINVAL, "bad blob magic");
    // (a blob of another packing version would load and compute wrong results: fold.py BLOB_VERSION)
    if (h->version != kBlobVersion)
        return fail(NHANS_EINVAL, "the folded blob has packing version " + std::to_string(h->version) + ", this library reads version " +
                                      std::to_string(kBlobVersion) + ": re-fold the weights (nhans_amd.fold.fold_weights)");
    if (h->total_bytes != nbytes || sizeof(BlobHeader) + (size_t)h->n_entries * sizeof(BlobEntry) > nbytes)
        return fail(NHANS_EINVAL, "blob size mismatch");
    HIP_TRY(hipSetDevice(device_id));
    nhans_ctx* c = new nhans_ctx();
    c->kind = model_kind;
    c->device = device_id;
    c->tower = tower_geometry();
    c->stack = main_geometry();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->blob_dev), nbytes);
    if (e != hipSuccess) { delete c; return fail(NHANS_ENOMEM, "hipMalloc for weights failed"); }
    c->blob_bytes = nbytes;
    e = hipMemcpy(c->blob_dev, blob, nbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { nhans_destroy(c); return fail(NHANS_EHIP, "weight upload failed"); }
    e = hipHostMalloc(reinterpret_cast<void**>(&c->pin), c->pin_bytes, hipHostMallocDefault);
    if (e != hipSuccess) { nhans_destroy(c); return fail(NHANS_ENOMEM, "pinned staging allocation failed"); }
    e = hipMalloc(reinterpret_cast<void**>(&c->kcounter), c->kcounter_n * sizeof(int));
    if (e == hipSuccess) e = hipMemset(c->kcounter, 0, c->kcounter_n * sizeof(int));
    if (e != hipSuccess) { nhans_destroy(c); return fail(NHANS_ENOMEM, "split-K ticket allocation failed"); }
    e = hipMalloc(reinterpret_cast<void**>(&c->status_dev), sizeof(int));
    if (e == hipSuccess) e = hipMemset(c->status_dev, 0, sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->amax_dev), kNumAct * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(c->amax_dev, 0, kNumAct * sizeof(unsigned));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->tail_ev, hipEventDisableTiming);
    if (e != hipSuccess) { nhans_destroy(c); return fail(NHANS_EHIP, "status word / ordering event creation failed"); }
    const BlobEntry* ent = reinterpret_cast<const BlobEntry*>(static_cast<const char*>(blob) + sizeof(BlobHeader));
    for (uint32_t i = 0; i < h->n_entries; ++i) {
        if (ent[i].offset % 16 || ent[i].offset + ent[i].nfloats * 4 > nbytes) {
            nhans_destroy(c); return fail(NHANS_EINVAL, "blob entry out of range");
        }
        std::string name(ent[i].name, strnlen(ent[i].name, sizeof ent[i].name));
        c->arr[name] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(c->blob_dev) + ent[i].offset);
        c->arr_n[name] = ent[i].nfloats;
    }
    // conditioning columns: conv order m0.c1, m0.c2, m1.c1, ...
    int off = 0;
    for (int b = 0; b < 8; ++b) for (int j = 0; j < 2; ++j) { c->cond_off.push_back(off); off += c->stack[b].cout; }
    c->cond_cols = off;
    // every array the launch sequences will dereference must be present with the right size
    std::vector<std::pair<std::string, size_t>> need = {
        {"tw400", 800}, {"window", 400}, {"wsyn", 400}, {"zero", 16384},
        {"cond.w", (size_t)2 * kEmb * off}, {"cond.base", (size_t)off},
        {"head.conv.wpk", (size_t)5 * 512 * 512}, {"head.conv.cb", 512},
        {"head.dense.wpk", (size_t)26 * 512 * 256}, {"head.dense.cb", 256}, {"head.dense.idw", 256}};
    for (int b = 0; b < 4; ++b) {
        const BlockGeo& g = c->tower[b];
        const std::string p = "t" + std::to_string(b);
        const size_t k2 = (size_t)g.kh * g.kw * g.cout * g.cout;
        if (b == 0) { need.push_back({p + ".c1.w", (size_t)g.kh * g.kw * 64}); need.push_back({p + ".c2.idw", (size_t)g.cout}); }
        else { need.push_back({p + ".c1.wpk", (size_t)g.kh * g.kw * g.cin * g.cout}); need.push_back({p + ".c2.wpk_t", (size_t)g.cin * g.cout}); }
        need.push_back({p + ".c1.cb", (size_t)g.cout});
        need.push_back({p + ".c2.wpk", k2});
        need.push_back({p + ".c2.cb", (size_t)g.cout});
    }
    for (int b = 0; b < 8; ++b) {
        const BlockGeo& g = c->stack[b];
        const std::string p = "m" + std::to_string(b);
        if (b == 0) need.push_back({p + ".c1.w", (size_t)g.kh * g.kw * 64});
        else need.push_back({p + ".c1.wpk", (size_t)g.kh * g.kw * g.cin * g.cout});
        need.push_back({p + ".c2.wpk", (size_t)g.kh * g.kw * g.cout * g.cout});
        if (b > 0 && g.cin != g.cout) need.push_back({p + ".c2.wpk_t", (size_t)g.cin * g.cout});
        need.push_back({p + ".c2.idw", (size_t)g.cout});
        for (const char* cv : {".c1", ".c2"}) {
            need.push_back({p + cv + ".tf", (size_t)g.hout * g.wout * g.cout});
        }
    }
    for (const auto& kv : need) {
        auto it = c->arr_n.find(kv.first);
        if (it == c->arr_n.end() || it->second != kv.second) {
            std::string msg = "folded blob: array '" + kv.first + "' missing or wrong size (want " +
                              std::to_string(kv.second) + ")";
            nhans_destroy(c);
            return fail(NHANS_EINVAL, msg);
        }
    }
    if (act_exp) {
        // (exponents a previous context calibrated for this very blob -- the caller's cache vouches for that: no pass)
        std::copy(act_exp, act_exp + kNumAct, c->act_exp);
        tie_exponents(c);
    } else if (c->A("head.dense.wpk_h")) {
        const int rc = calibrate_builtin(c);
        if (rc) { nhans_destroy(c); return rc; }
    }
    *out = c;
    return NHANS_OK;
}

void nhans_destroy(nhans_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : c->prof)
        for (auto& ev : kv.second.pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (hipEvent_t ev : c->event_pool) (void)hipEventDestroy(ev);
    if (c->tail_ev) (void)hipEventDestroy(c->tail_ev);
    if (c->status_dev) (void)hipFree(c->status_dev);
    if (c->amax_dev) (void)hipFree(c->amax_dev);
    for (auto& kv : c->rs_tab) (void)hipFree(kv.second);
    if (c->ws) (void)hipFree(c->ws);
    if (c->kscratch) (void)hipFree(c->kscratch);
    if (c->kcounter) (void)hipFree(c->kcounter);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->blob_dev) (void)hipFree(c->blob_dev);
    delete c;
}

int nhans_set_option(nhans_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return fail(NHANS_EINVAL, "null argument");
    const std::string k(key);
    if (k == "frames_per_chunk") {
        // the fast conv kernels address a tensor with 32-bit element offsets: the largest one of a pass
        // (frames x 35 x 201 x 64) must stay below 2^31 elements, i.e. at most 4,769 frames; above that every
        // layer would silently fall back to the slow kernel, far above it M = frames x Ho x Wo overflows int
        if (value < 1 || value > kMaxFramesPerChunk)
            return fail(NHANS_EINVAL, "frames_per_chunk must be in [1, " + std::to_string(kMaxFramesPerChunk) + "]");
        c->frames_per_chunk = value;
    }
    else if (k == "contexts_per_chunk") { if (value < 1) return fail(NHANS_EINVAL, "contexts_per_chunk < 1"); c->contexts_per_chunk = (int)value; }
    else if (k == "lookahead") {
        if (value < 0 || value > kCenter) return fail(NHANS_EINVAL, "lookahead must be in [0, " + std::to_string(kCenter) + "] frames");
        c->lookahead = (int)value;
    }
    else if (k == "profile") c->profile = value != 0;
    else if (k == "debug_cycles_ptr") {
        if (!kDev) return fail(NHANS_EINVAL, "debug_cycles_ptr exists only in a NHANS_DEV build (make DEV=1)");
        c->dbg = reinterpret_cast<long long*>(static_cast<intptr_t>(value));
    }
    else if (k == "epilogue_wide") c->epi8 = value != 0;
    else if (k == "consumer_interleave") {
        if (value < 0 || value > 2) return fail(NHANS_EINVAL, "consumer_interleave must be 0, 1 or 2");
        c->ilv = (int)value;
    }
    else if (k == "conv_variant") {
        if (value < -1 || value > 2) return fail(NHANS_EINVAL, "conv_variant must be -1 (auto), 0, 1 or 2");
        c->conv_variant = (int)value;
    }
    else if (k == "calibrate") {
        if (value < 0 || value > 3) return fail(NHANS_EINVAL, "calibrate must be 1 (start), 0 (stop, set), 2 (stop, raise only) or 3 (stop, discard)");
        int rc = check_ctx(c); if (rc) return rc;
        if (value == 1) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipMemset(c->amax_dev, 0, kNumAct * sizeof(unsigned)));
            c->calibrating = true;
        } else {
            if (!c->calibrating) return fail(NHANS_EINVAL, "calibrate: no bracket is open");
            if (value == 3) { c->calibrating = false; return NHANS_OK; }     // (the pass failed: nothing was learnt)
            return finish_calibration(c, value == 2);
        }
    }
    else if (k == "winograd") c->wino = value != 0;
    else if (k == "winograd_f32_tensors") c->wino_f32 = (value == 2 || value == 3) ? (int)value : value != 0;
    else if (k == "split_k") c->split_k = value != 0;
    else if (k == "stream_1x1") c->stream_1x1 = value != 0;
    else if (k == "precision") {
        if (value != 0 && value != 1) return fail(NHANS_EINVAL, "precision must be 0 (f32) or 1 (f16x3)");
        if (value == 1 && !c->A("head.dense.wpk_h"))
            return fail(NHANS_EINVAL, "the folded blob carries no split-f16 weights");
        c->prec = (int)value;
    }
    else return fail(NHANS_EINVAL, "unknown option " + k);
    return NHANS_OK;
}

int nhans_set_activation_exponents(nhans_ctx* c, const int* e, int n) {
    if (!c || !e || n != kNumAct) return fail(NHANS_EINVAL, "activation exponents: need NHANS_NUM_ACTIVATIONS values");
    for (int i = 0; i < n; ++i)
        if (e[i] < -60 || e[i] > 60) return fail(NHANS_EINVAL, "activation exponent outside [-60, 60]");
    std::copy(e, e + n, c->act_exp);
    tie_exponents(c);
    return NHANS_OK;
}

int nhans_get_activation_exponents(nhans_ctx* c, int* e_out, int n) {
    if (!c || !e_out || n != kNumAct) return fail(NHANS_EINVAL, "activation exponents: need NHANS_NUM_ACTIVATIONS values");
    std::copy(c->act_exp, c->act_exp + n, e_out);
    return NHANS_OK;
}

int nhans_get_activation_amax(nhans_ctx* c, float* amax_out, int n) {
    if (!c || !amax_out || n != kNumAct) return fail(NHANS_EINVAL, "activation maxima: need NHANS_NUM_ACTIVATIONS values");
    std::copy(c->act_amax, c->act_amax + n, amax_out);
    return NHANS_OK;
}

size_t nhans_workspace_bytes(nhans_ctx* c, int64_t total_frames, int nclips) {
    if (!c) return 0;
    const int64_t wf = std::min<int64_t>(c->frames_per_chunk, std::max<int64_t>(total_frames, 1));
    size_t b = stack_ws_bytes(c, total_frames, nclips, wf);
    b = std::max(b, 3 * ws_size(tower_buf_floats(c), 4));
    b += 4 * ws_size((size_t)total_frames * kBins, 4);                       // logmag, phase, denoised, logits
    b += ws_size((size_t)2 * nclips * kCtxFrames * kBins, 4) + ws_size((size_t)2 * nclips * kEmb, 4);
    b += 1 << 20;
    return b;
}

static int stft_features_body(nhans_ctx* c, const float* wav, const int64_t* soff, int nclips, int maxf,
                        float* logmag, float* phase, void* stream) {
    int rc = NHANS_OK;
    if (!wav || !soff || !logmag || nclips < 0) return fail(NHANS_EINVAL, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nb = stft_blocks(soff, nclips, maxf);
    rc = ws_reserve(c, ws_size(2 * (nclips + 1), 8) + ws_size(2 * nb, 4)); if (rc) return rc;
    int64_t* tabs = ws_take<int64_t>(c, 2 * (nclips + 1));
    int* blocks = ws_take<int>(c, 2 * nb);
    return stft_impl(c, wav, soff, nclips, maxf, logmag, phase, tabs, blocks, nullptr, s);
}

int nhans_stft_features(nhans_ctx* c, const float* wav, const int64_t* soff, int nclips, int maxf,
                        float* logmag, float* phase, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(stft_features_body(c, wav, soff, nclips, maxf, logmag, phase, stream));
}

static int embed_body(nhans_ctx* c, const float* ctx_lm, int n, float* emb_out, void* stream) {
    int rc = NHANS_OK;
    if (!ctx_lm || !emb_out || n < 0) return fail(NHANS_EINVAL, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nb = tower_buf_floats(c);
    rc = ws_reserve(c, 3 * ws_size(nb, 4)); if (rc) return rc;
    float* X = ws_take<float>(c, nb); float* A = ws_take<float>(c, nb); float* Y = ws_take<float>(c, nb);
    return embed_impl(c, ctx_lm, n, emb_out, X, A, Y, s);
}

int nhans_embed(nhans_ctx* c, const float* ctx_lm, int n, float* emb_out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(embed_body(c, ctx_lm, n, emb_out, stream));
}

static int mask_net_body(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                   const float* eb, float* logits, float* denoised, void* stream) {
    int rc = NHANS_OK;
    if (!logmag || !foff || !ea || !eb || !denoised || nclips < 1) return fail(NHANS_EINVAL, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = foff[nclips];
    if (total <= 0) return NHANS_OK;
    const int64_t wf = std::min<int64_t>(c->frames_per_chunk, total);
    rc = ws_reserve(c, stack_ws_bytes(c, total, nclips, wf)); if (rc) return rc;
    StackBufs sb;
    stack_take(c, total, nclips, wf, &sb);
    return mask_net_impl(c, logmag, foff, nclips, ea, eb, logits, denoised, sb, wf, s);
}

int nhans_mask_net(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                   const float* eb, float* logits, float* denoised, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(mask_net_body(c, logmag, foff, nclips, ea, eb, logits, denoised, stream));
}

static int debug_block_output_body(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                             const float* eb, int64_t frame0, int nframes, int block, float* out, void* stream) {
    int rc = NHANS_OK;
    if (!logmag || !foff || !ea || !eb || !out || block < 0 || block > 8) return fail(NHANS_EINVAL, "bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = foff[nclips];
    if (frame0 < 0 || frame0 + nframes > total) return fail(NHANS_EINVAL, "frame range outside batch");
    rc = ws_reserve(c, stack_ws_bytes(c, total, nclips, nframes)); if (rc) return rc;
    StackBufs sb;
    stack_take(c, total, nclips, nframes, &sb);
    rc = h2d(c, sb.foff_dev, foff, (nclips + 1) * sizeof(int64_t), s); if (rc) return rc;
    launch_frame_index(sb.foff_dev, nclips, total, c->lookahead, sb.f_clip, sb.f_t, sb.f_T, s);
    launch_cond(ea, eb, nclips, c->A("cond.w"), c->A("cond.base"), c->cond_cols, sb.cb_all, s);
    const float* res = run_stack_chunk(c, logmag, nullptr, sb, frame0, nframes, block + 1, s);
    size_t per;
    if (block == 8) per = (size_t)26 * 512;
    else per = (size_t)c->stack[block].hout * c->stack[block].wout * c->stack[block].cout;
    if (c->prec && block < 8 && stored_f32(c, c->last_plan, block, 1)) launch_scale_copy(res, per * nframes, c->up(SA(block, 1)), out, s);
    else if (c->prec) launch_unsplit(res, (int64_t)nframes * (int64_t)(per / (block == 8 ? 512 : c->stack[block].cout)),
                                block == 8 ? 512 : c->stack[block].cout, c->up(block == 8 ? kActHead : SA(block, 1)), out, s);
    else HIP_TRY(hipMemcpyAsync(out, res, per * nframes * 4, hipMemcpyDeviceToDevice, s));
    return NHANS_OK;
}

int nhans_debug_block_output(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                             const float* eb, int64_t frame0, int nframes, int block, float* out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(debug_block_output_body(c, logmag, foff, nclips, ea, eb, frame0, nframes, block, out, stream));
}

// Any stored tensor of the stack + head (index 8 .. 24) for frames [frame0, frame0 + nframes): the production launch
// sequence -- one plan for the whole stack, frames_per_chunk frame windows per pass counted from frame0 -- up to the block
// that writes it; the tap() point of that tensor converts every chunk's finished buffer.
static int debug_activation_body(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                                 const float* eb, int64_t frame0, int nframes, int index, float* out, void* stream) {
    int rc = NHANS_OK;
    if (!logmag || !foff || !ea || !eb || !out || nclips < 1 || nframes < 1) return fail(NHANS_EINVAL, "bad argument");
    if (index < SA(0, 0) || index >= kNumAct)
        return fail(NHANS_EINVAL, "activation index outside the stack's 8 .. " + std::to_string(kNumAct - 1) + " (tower tensors: nhans_debug_tower_activation)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = foff[nclips];
    if (frame0 < 0 || frame0 + nframes > total) return fail(NHANS_EINVAL, "frame range outside batch");
    const int64_t wf = std::min<int64_t>(c->frames_per_chunk, nframes);
    rc = ws_reserve(c, stack_ws_bytes(c, total, nclips, wf)); if (rc) return rc;
    StackBufs sb;
    stack_take(c, total, nclips, wf, &sb);
    rc = h2d(c, sb.foff_dev, foff, (nclips + 1) * sizeof(int64_t), s); if (rc) return rc;
    launch_frame_index(sb.foff_dev, nclips, total, c->lookahead, sb.f_clip, sb.f_t, sb.f_T, s);
    launch_cond(ea, eb, nclips, c->A("cond.w"), c->A("cond.base"), c->cond_cols, sb.cb_all, s);
    const int upto = index == kActHead ? 9 : (index - SA(0, 0)) / 2 + 1;
    c->cap_idx = index; c->cap_out = out;
    for (int64_t g0 = frame0; g0 < frame0 + nframes; g0 += wf) {
        run_stack_chunk(c, logmag, nullptr, sb, g0, (int)std::min<int64_t>(wf, frame0 + nframes - g0), upto, s);
        if (launch_error_pending()) break;
    }
    c->cap_idx = -1; c->cap_out = nullptr;
    return NHANS_OK;
}

int nhans_debug_activation(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                           const float* eb, int64_t frame0, int nframes, int index, float* out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(debug_activation_body(c, logmag, foff, nclips, ea, eb, frame0, nframes, index, out, stream));
}

// Any stored tensor of the embedding tower (index 0 .. 7) for n context images: nhans_embed's own launches (chunks of
// contexts_per_chunk images, the pooled embeddings go to the workspace) with the tap() point of that tensor copying out.
static int debug_tower_activation_body(nhans_ctx* c, const float* ctx_lm, int n, int index, float* out, void* stream) {
    int rc = NHANS_OK;
    if (!ctx_lm || !out || n < 1) return fail(NHANS_EINVAL, "bad argument");
    if (index < 0 || index >= SA(0, 0))
        return fail(NHANS_EINVAL, "activation index outside the tower's 0 .. 7 (stack tensors: nhans_debug_activation)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nb = tower_buf_floats(c);
    rc = ws_reserve(c, 3 * ws_size(nb, 4) + ws_size((size_t)n * kEmb, 4)); if (rc) return rc;
    float* X = ws_take<float>(c, nb); float* A = ws_take<float>(c, nb); float* Y = ws_take<float>(c, nb);
    float* emb = ws_take<float>(c, (size_t)n * kEmb);
    c->cap_idx = index; c->cap_out = out;
    rc = embed_impl(c, ctx_lm, n, emb, X, A, Y, s);
    c->cap_idx = -1; c->cap_out = nullptr;
    return rc;
}

int nhans_debug_tower_activation(nhans_ctx* c, const float* ctx_lm, int n, int index, float* out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(debug_tower_activation_body(c, ctx_lm, n, index, out, stream));
}

static int istft_body(nhans_ctx* c, const float* logmag, const float* phase, const int64_t* foff, int nclips,
                const int64_t* ooff, float* wav_out, void* stream) {
    int rc = NHANS_OK;
    if (!logmag || !phase || !foff || !ooff || !wav_out) return fail(NHANS_EINVAL, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nb = istft_blocks(foff, nclips);
    rc = ws_reserve(c, ws_size(2 * (nclips + 1), 8) + ws_size(2 * nb, 4)); if (rc) return rc;
    int64_t* tabs = ws_take<int64_t>(c, 2 * (nclips + 1));
    int* blocks = ws_take<int>(c, 2 * nb);
    return istft_impl(c, logmag, phase, foff, nclips, ooff, wav_out, tabs, blocks, s);
}

int nhans_istft(nhans_ctx* c, const float* logmag, const float* phase, const int64_t* foff, int nclips,
                const int64_t* ooff, float* wav_out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(istft_body(c, logmag, phase, foff, nclips, ooff, wav_out, stream));
}

static int enhance_clips_body(nhans_ctx* c, const float* mix, const int64_t* moff, int nclips, const float* ca,
                        const int64_t* caoff, const float* cbw, const int64_t* cboff, float* den_wav,
                        float* mixed_wav, float* logmag_out, float* phase_out, float* logits_out, float* emb_out,
                        void* stream) {
    int rc = NHANS_OK;
    if (!mix || !moff || !ca || !caoff || !cbw || !cboff || !den_wav || nclips < 1)
        return fail(NHANS_EINVAL, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<int64_t> foff(nclips + 1, 0);
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = moff[i + 1] - moff[i];
        if (n >= kWin && (n - kWin) % kHop != 0)
            return fail(NHANS_EINVAL, "mixture clip " + std::to_string(i) + " is not trimmed to a whole frame count");
        foff[i + 1] = foff[i] + nhans_num_frames(n);
    }
    const int64_t total = foff[nclips];
    const int64_t wf = std::min<int64_t>(c->frames_per_chunk, std::max<int64_t>(total, 1));
    // workspace plan
    const size_t nb_mix = stft_blocks(moff, nclips, 0), nb_ca = stft_blocks(caoff, nclips, kCtxFrames),
                 nb_cb = stft_blocks(cboff, nclips, kCtxFrames), nb_is = istft_blocks(foff.data(), nclips);
    const size_t nblk = std::max(std::max(nb_mix, nb_ca), std::max(nb_cb, nb_is));
    size_t bytes = 4 * ws_size((size_t)total * kBins, 4) + ws_size((size_t)2 * nclips * kCtxFrames * kBins, 4) +
                   ws_size((size_t)2 * nclips * kEmb, 4) + 4 * ws_size(2 * (nclips + 1), 8) + 4 * ws_size(2 * nblk, 4);
    bytes += std::max(stack_ws_bytes(c, total, nclips, wf), 3 * ws_size(tower_buf_floats(c), 4));
    rc = ws_reserve(c, bytes); if (rc) return rc;
    float* lm = ws_take<float>(c, (size_t)total * kBins);
    float* ph = ws_take<float>(c, (size_t)total * kBins);
    float* den = ws_take<float>(c, (size_t)total * kBins);
    float* lg = ws_take<float>(c, (size_t)total * kBins);
    float* ctxlm = ws_take<float>(c, (size_t)2 * nclips * kCtxFrames * kBins);
    float* emb = ws_take<float>(c, (size_t)2 * nclips * kEmb);
    int64_t* tabs[4]; int* blks[4];
    for (int i = 0; i < 4; ++i) { tabs[i] = ws_take<int64_t>(c, 2 * (nclips + 1)); blks[i] = ws_take<int>(c, 2 * nblk); }
    const size_t mark = c->ws_top;

    rc = stft_impl(c, mix, moff, nclips, 0, lm, ph, tabs[0], blks[0], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, ca, caoff, nclips, kCtxFrames, ctxlm, nullptr, tabs[1], blks[1], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, cbw, cboff, nclips, kCtxFrames, ctxlm + (size_t)nclips * kCtxFrames * kBins, nullptr, tabs[2],
                   blks[2], nullptr, s);
    if (rc) return rc;
    {
        const size_t nb = tower_buf_floats(c);
        float* X = ws_take<float>(c, nb); float* A = ws_take<float>(c, nb); float* Y = ws_take<float>(c, nb);
        rc = embed_impl(c, ctxlm, 2 * nclips, emb, X, A, Y, s); if (rc) return rc;
    }
    if (total > 0) {
        c->ws_top = mark;
        StackBufs sb;
        stack_take(c, total, nclips, wf, &sb);
        rc = mask_net_impl(c, lm, foff.data(), nclips, emb, emb + (size_t)nclips * kEmb, lg, den, sb, wf, s);
        if (rc) return rc;
        rc = istft_impl(c, den, ph, foff.data(), nclips, moff, den_wav, tabs[3], blks[3], s); if (rc) return rc;
        if (mixed_wav) {
            // tabs/blks[3] are reused: same stream, so the first launch has consumed them in order
            rc = istft_impl(c, lm, ph, foff.data(), nclips, moff, mixed_wav, tabs[3], blks[3], s); if (rc) return rc;
        }
        if (logmag_out) HIP_TRY(hipMemcpyAsync(logmag_out, lm, (size_t)total * kBins * 4, hipMemcpyDeviceToDevice, s));
        if (phase_out) HIP_TRY(hipMemcpyAsync(phase_out, ph, (size_t)total * kBins * 4, hipMemcpyDeviceToDevice, s));
        if (logits_out) HIP_TRY(hipMemcpyAsync(logits_out, lg, (size_t)total * kBins * 4, hipMemcpyDeviceToDevice, s));
    }
    if (emb_out) HIP_TRY(hipMemcpyAsync(emb_out, emb, (size_t)2 * nclips * kEmb * 4, hipMemcpyDeviceToDevice, s));
    return NHANS_OK;
}

int nhans_enhance_clips(nhans_ctx* c, const float* mix, const int64_t* moff, int nclips, const float* ca,
                        const int64_t* caoff, const float* cbw, const int64_t* cboff, float* den_wav,
                        float* mixed_wav, float* logmag_out, float* phase_out, float* logits_out, float* emb_out,
                        void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(enhance_clips_body(c, mix, moff, nclips, ca, caoff, cbw, cboff, den_wav, mixed_wav, logmag_out, phase_out, logits_out, emb_out, stream));
}

int nhans_take_status(nhans_ctx* c, int* flags_out, void* stream) {
    int rc = check_ctx(c); if (rc) return rc;
    if (!flags_out) return fail(NHANS_EINVAL, "null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the kernels that set the bits may have run on another stream than the one given here: order the
    // read-and-clear behind the context's last call, as every hot-path entry point does (struct Call)
    if (c->have_tail && c->last_stream != s) HIP_TRY(hipStreamWaitEvent(s, c->tail_ev, 0));
    int flags = 0;
    HIP_TRY(hipMemcpyAsync(&flags, c->status_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(c->status_dev, 0, sizeof(int), s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hipEventRecord(c->tail_ev, s) == hipSuccess) { c->have_tail = true; c->last_stream = s; }   // the clear is part of the order
    *flags_out = flags;
    return NHANS_OK;
}

int nhans_debug_launch_probe(size_t dynamic_lds_bytes, void* stream) {
    (void)take_launch_error(nullptr);
    static unsigned long long probe_devices = 0;
    if (dynamic_lds_bytes > 65536)
        set_max_dynamic_lds(reinterpret_cast<const void*>(&launch_probe_kernel), dynamic_lds_bytes, &probe_devices, "launch_probe");
    // (the launch is attempted even if the attribute was refused: both failures must surface)
    NHANS_LAUNCH("launch_probe", launch_probe_kernel, dim3(1), dim3(64), dynamic_lds_bytes, static_cast<hipStream_t>(stream),
                 static_cast<int*>(nullptr));
    return launch_status();
}

uint32_t nhans_crc32c(uint32_t crc, const void* data, size_t n) {
    // slicing-by-8 over the reflected Castagnoli polynomial 0x82F63B78
    static const struct Tab {
        uint32_t t[8][256];
        Tab() {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
                t[0][i] = c;
            }
            for (uint32_t i = 0; i < 256; ++i)
                for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
        }
    } T;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint32_t c = ~crc;
    while (n >= 8) {
        uint32_t lo, hi;
        std::memcpy(&lo, p, 4);
        std::memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T.t[7][lo & 0xFF] ^ T.t[6][(lo >> 8) & 0xFF] ^ T.t[5][(lo >> 16) & 0xFF] ^ T.t[4][lo >> 24] ^
            T.t[3][hi & 0xFF] ^ T.t[2][(hi >> 8) & 0xFF] ^ T.t[1][(hi >> 16) & 0xFF] ^ T.t[0][hi >> 24];
        p += 8;
        n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return ~c;
}

int nhans_profile_reset(nhans_ctx* c) {
    if (!c) return fail(NHANS_EINVAL, "null context");
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : c->prof)
        for (auto& ev : kv.second.pending) { c->event_pool.push_back(ev.first); c->event_pool.push_back(ev.second); }
    c->prof.clear();
    return NHANS_OK;
}

int nhans_profile_json(nhans_ctx* c, char* buf, size_t buflen) {
    if (!c) return fail(NHANS_EINVAL, "null context");
    (void)hipSetDevice(c->device);
    std::string js = "{";
    bool first = true;
    for (auto& kv : c->prof) {
        ProfEntry& e = kv.second;
        for (auto& ev : e.pending) {
            (void)hipEventSynchronize(ev.second);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) e.ms += ms;
            c->event_pool.push_back(ev.first);
            c->event_pool.push_back(ev.second);
        }
        e.pending.clear();
        char line[384];
        snprintf(line, sizeof line, "%s\"%s\": {\"calls\": %d, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e, \"mfma_flops\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), e.calls, e.ms, e.flops, e.bytes, e.mfma);
        js += line;
        first = false;
    }
    js += "}";
    if (buf && buflen) {
        const size_t n = std::min(buflen - 1, js.size());
        std::memcpy(buf, js.data(), n);
        buf[n] = 0;
    }
    return (int)js.size();
}

}  // extern "C"

// ---- online enhancement (include/nhans_hip.h: nhans_online_*) ----------------------------------------------------------
// Synthesis restarts at frame S0(P): the offline iSTFT kernel's bits depend on where a frame pair falls in its run of
// kIstftHopsPerBlock hops (the pairs of a run are different unrolled copies of the transform, which the compiler may
// contract differently: ~1e-7), so the staged clip of a push starts on that grid of the stream's frames, at or before
// P - 2 (the first frame under the first sample not emitted yet).
// State of one online stream in one slot, floats: the unconsumed samples [160 T, N) (< 400), the log-magnitude and phase
// rows of frames [lo, T), lo = max(0, min(R - 17, S0(P))) (<= 41: the history of the next ready frame's window, the
// look-ahead rows that exist, every row the iSTFT still needs), and the denoised rows [S0(P), R) (<= 24: computed, not
// yet synthesised, and those the next synthesis restarts from).  A push reads slot `cur` and writes the other slot
// whole; nhans_online_rewind flips back.
// nhans_online_restart clears nothing on the device: a stream of N = 0, T = 0 has no carried samples, lo = S0 = R = 0 and
// no row below T, so its first push reads nothing of slot `cur` (every run taken from the state is empty) and writes the
// other slot from the push alone.  The same holds for the slots of nhans_online_open_slots, whose state is never filled.
namespace {
int slot_check(int S, int slot, const char* fn) {
    if (slot < 0 || slot >= S)
        return fail(NHANS_EINVAL, std::string(fn) + ": slot " + std::to_string(slot) + " outside [0, " + std::to_string(S) + ")");
    return NHANS_OK;
}

// What a push of cnt samples (en: and the end) to stream i may not be, for the three streaming objects and their
// out_counts: `noun` is what the object calls a stream ("stream" / "slot"), `ended` the stream's flag, `uncond` non-null
// where the slot has no conditioning and the call refuses samples for such a slot (it names the calls that set one),
// max_cnt the most samples one push of the object takes.
constexpr int64_t kMaxResampleClip = ((int64_t)1 << 31) - 1, kNoPushCap = std::numeric_limits<int64_t>::max();
int push_check(const char* fn, const char* noun, int i, int64_t cnt, bool en, bool ended, const char* uncond, int64_t max_cnt) {
    const std::string who = std::string(fn) + ": " + noun + " " + std::to_string(i);
    if (cnt < 0) return fail(NHANS_EINVAL, who + " has a negative sample count");
    if (ended && (cnt > 0 || en)) return fail(NHANS_EINVAL, who + " has ended");
    if (uncond && (cnt > 0 || en))
        return fail(NHANS_EINVAL, std::string(fn) + ": slot " + std::to_string(i) + " has no conditioning yet (" + uncond + ")");
    if (cnt > max_cnt) return fail(NHANS_EINVAL, std::string(fn) + ": push too large for one call (split it)");
    return NHANS_OK;
}

constexpr int kOnRows = 2 * kCenter + kIstftHopsPerBlock - 14;  // 42 >= 17 + 24
constexpr int kOnDenRows = kIstftHopsPerBlock + 2;              // 24
constexpr size_t kOnSamp = 0, kOnLm = kWin, kOnPh = kOnLm + (size_t)kOnRows * kBins, kOnDen = kOnPh + (size_t)kOnRows * kBins;
constexpr size_t kOnSlot = (kOnDen + (size_t)kOnDenRows * kBins + 63) & ~(size_t)63;   // 22,144 floats = 88.6 KB
int64_t on_s0(int64_t P) { return std::max<int64_t>(0, P - 2) / kIstftHopsPerBlock * kIstftHopsPerBlock; }
int64_t on_lo(int64_t R, int64_t P) { return std::max<int64_t>(0, std::min<int64_t>(R - kCenter, on_s0(P))); }

struct OnStream {
    int64_t N = 0, T = 0;
    bool ended = false;
};
// frames that are computed (their L look-ahead rows exist) / frames whose samples are final, for a stream of T frames with
// look-ahead L.  on_lo keeps its form: the window still reaches 17 rows BACK from the next ready frame R = T - L, so
// T - lo = L + (R - lo) <= L + max(17, R - S0) <= 41 rows and R - S0 <= 24 for every L <= 17.
int64_t on_ready(int64_t T, bool ended, int L) { return ended ? T : std::max<int64_t>(0, T - L); }
int64_t on_paired(int64_t T, bool ended, int L) { return ended ? T : on_ready(T, false, L) & ~(int64_t)1; }
int64_t on_emitted(int64_t T, bool ended, int L) {
    if (!ended) return (int64_t)kHop * on_paired(T, false, L);
    return T == 0 ? 0 : (T - 1) * kHop + kWin;
}
}  // namespace

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
    float* slot(int k, int i) const { return state + ((size_t)k * S + i) * kOnSlot; }
};

namespace {

// final samples a push of cnt samples (en: and the end) to stream i makes
int64_t online_emit_count(const nhans_online* o, int i, int64_t cnt, bool en) {
    const OnStream& q = o->st[i];
    return on_emitted(nhans_num_frames(q.N + cnt), q.ended || en, o->la[i]) - on_emitted(q.T, q.ended, o->la[i]);
}

// The last push undone (nhans_online_rewind, and a live push whose later stage did not go out).  The rings keep what the
// undone push wrote: vlo moved to max(vlo, N - 32,240) when its copies went out and stays.
void online_undo(nhans_online* o) {
    o->st = o->prev;
    o->cur = 1 - o->cur;
    o->can_rewind = false;
}

// The object and its device memory; on failure nothing is left allocated.
int online_alloc(nhans_ctx* c, int S, int want_mixed, bool conditioned, const char* fn, nhans_online** out) {
    nhans_online* o = new nhans_online();
    o->c = c; o->device = c->device; o->S = S; o->mixed = want_mixed != 0;
    o->st.assign(S, OnStream()); o->prev = o->st;
    o->cond.assign(S, conditioned ? 1 : 0);
    o->la.assign(S, kCenter);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->emb), (size_t)2 * S * kEmb * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->state), (size_t)2 * S * kOnSlot * 4);
    if (e != hipSuccess) {
        if (o->emb) (void)hipFree(o->emb);
        delete o;
        return fail(NHANS_ENOMEM, std::string(fn) + ": hipMalloc failed: " + hipGetErrorString(e));
    }
    *out = o;
    return NHANS_OK;
}

int online_open_body(nhans_ctx* c, int S, const float* ca, const int64_t* caoff, const float* cbw, const int64_t* cboff,
                     int want_mixed, hipStream_t s, nhans_online** out) {
    if (!out) return fail(NHANS_EINVAL, "null argument");
    *out = nullptr;
    if (S < 1) return fail(NHANS_EINVAL, "nhans_online_open: nstreams must be >= 1");
    if (!ca || !caoff || !cbw || !cboff) return fail(NHANS_EINVAL, "null argument");
    const size_t nb = std::max(stft_blocks(caoff, S, kCtxFrames), stft_blocks(cboff, S, kCtxFrames));
    const size_t tb = tower_buf_floats(c);
    int rc = ws_reserve(c, ws_size((size_t)2 * S * kCtxFrames * kBins, 4) + 2 * ws_size(2 * (S + 1), 8) +
                               2 * ws_size(2 * nb, 4) + 3 * ws_size(tb, 4));
    if (rc) return rc;
    float* ctxlm = ws_take<float>(c, (size_t)2 * S * kCtxFrames * kBins);
    int64_t* tabs[2]; int* blks[2];
    for (int i = 0; i < 2; ++i) { tabs[i] = ws_take<int64_t>(c, 2 * (S + 1)); blks[i] = ws_take<int>(c, 2 * nb); }
    float* X = ws_take<float>(c, tb); float* A = ws_take<float>(c, tb); float* Y = ws_take<float>(c, tb);
    rc = stft_impl(c, ca, caoff, S, kCtxFrames, ctxlm, nullptr, tabs[0], blks[0], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, cbw, cboff, S, kCtxFrames, ctxlm + (size_t)S * kCtxFrames * kBins, nullptr, tabs[1], blks[1], nullptr, s);
    if (rc) return rc;
    nhans_online* o = nullptr;
    rc = online_alloc(c, S, want_mixed, true, "nhans_online_open", &o); if (rc) return rc;
    rc = embed_impl(c, ctxlm, 2 * S, o->emb, X, A, Y, s);
    if (rc) { (void)hipFree(o->emb); (void)hipFree(o->state); delete o; return rc; }
    *out = o;
    return NHANS_OK;
}

int online_open_slots_body(nhans_ctx* c, int S, int want_mixed, hipStream_t s, nhans_online** out) {
    if (!out) return fail(NHANS_EINVAL, "nhans_online_open_slots: null argument");
    *out = nullptr;
    if (S < 1) return fail(NHANS_EINVAL, "nhans_online_open_slots: nslots must be >= 1");
    nhans_online* o = nullptr;
    int rc = online_alloc(c, S, want_mixed, false, "nhans_online_open_slots", &o); if (rc) return rc;
    // (the conditioning kernel of every pass reads all S row pairs: idle rows are zeros, not uninitialised memory)
    const hipError_t e = hipMemsetAsync(o->emb, 0, (size_t)2 * S * kEmb * 4, s);
    if (e != hipSuccess) {
        (void)hipFree(o->emb); (void)hipFree(o->state); delete o;
        return fail(NHANS_EHIP, std::string("nhans_online_open_slots: hipMemsetAsync: ") + hipGetErrorString(e));
    }
    *out = o;
    return NHANS_OK;
}

// Slot `slot` becomes an open stream of 0 samples (nhans_online_restart, nhans_live_restart): a new timeline, of which the
// ring holds nothing yet.
void online_restart_slot(nhans_online* o, int slot) {
    o->st[slot] = OnStream();
    if (o->ring) o->vlo[slot] = o->whi[slot] = 0;
    o->can_rewind = false;
}

// Rows `slot` (a) and S + `slot` (b) of the embeddings <- two [512] device rows, ordered on s after whatever made them.
// Frames already computed keep the conditioning they were computed with: *first_frame is the first that will not.
int online_set_rows(nhans_online* o, int slot, const float* row_a, const float* row_b, hipStream_t s, int64_t* first_frame) {
    HIP_TRY(hipMemcpyAsync(o->emb + (size_t)slot * kEmb, row_a, kEmb * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(o->emb + (size_t)(o->S + slot) * kEmb, row_b, kEmb * 4, hipMemcpyDeviceToDevice, s));
    o->cond[slot] = 1;
    o->can_rewind = false;
    if (first_frame) *first_frame = on_ready(o->st[slot].T, o->st[slot].ended, o->la[slot]);
    return NHANS_OK;
}

int online_set_context_body(nhans_online* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb_,
                            hipStream_t s, int64_t* first_frame) {
    nhans_ctx* c = o->c;
    int rc = slot_check(o->S, slot, "nhans_online_set_context"); if (rc) return rc;
    if (!ca || !cbw) return fail(NHANS_EINVAL, "nhans_online_set_context: null argument");
    if (na < 0 || nb_ < 0) return fail(NHANS_EINVAL, "nhans_online_set_context: negative sample count");
    const int64_t aoff[2] = {0, na}, boff[2] = {0, nb_};
    const size_t nb = std::max(stft_blocks(aoff, 1, kCtxFrames), stft_blocks(boff, 1, kCtxFrames));
    const size_t tb = tower_buf_floats(c);
    rc = ws_reserve(c, ws_size((size_t)2 * kCtxFrames * kBins, 4) + ws_size(2 * kEmb, 4) + 2 * ws_size(4, 8) +
                           2 * ws_size(2 * nb, 4) + 3 * ws_size(tb, 4));
    if (rc) return rc;
    float* ctxlm = ws_take<float>(c, (size_t)2 * kCtxFrames * kBins);
    float* rows = ws_take<float>(c, 2 * kEmb);
    int64_t* tabs[2]; int* blks[2];
    for (int i = 0; i < 2; ++i) { tabs[i] = ws_take<int64_t>(c, 4); blks[i] = ws_take<int>(c, 2 * nb); }
    float* X = ws_take<float>(c, tb); float* A = ws_take<float>(c, tb); float* Y = ws_take<float>(c, tb);
    rc = stft_impl(c, ca, aoff, 1, kCtxFrames, ctxlm, nullptr, tabs[0], blks[0], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, cbw, boff, 1, kCtxFrames, ctxlm + (size_t)kCtxFrames * kBins, nullptr, tabs[1], blks[1], nullptr, s);
    if (rc) return rc;
    // (the tower writes workspace rows, not the object's: a failure leaves the slot's conditioning as it was)
    rc = embed_impl(c, ctxlm, 2, rows, X, A, Y, s); if (rc) return rc;
    if (launch_error_pending()) return NHANS_OK;          // (reported by the entry point; the slot keeps its rows)
    return online_set_rows(o, slot, rows, rows + kEmb, s, first_frame);
}

int online_set_embeddings_body(nhans_online* o, int slot, const float* ea, const float* eb, hipStream_t s, int64_t* first_frame) {
    const int rc = slot_check(o->S, slot, "nhans_online_set_embeddings"); if (rc) return rc;
    if (!ea || !eb) return fail(NHANS_EINVAL, "nhans_online_set_embeddings: null argument");
    return online_set_rows(o, slot, ea, eb, s, first_frame);
}

// One push; see include/nhans_hip.h.  Host plan first (every count, offset and copy run), then the launches:
//   online_ingest   carried samples + new input -> wav staging (compact, one clip per stream)
//   online_stft     the newly complete frames -> new log-magnitude / phase rows (the offline STFT kernel)
//   online_assemble window source [lo, T_new) per stream, the ready frames' centre rows, synthesis staging from the state
//   stack + head    over the ready frames of all streams at once (per-frame first-row table: WinRows::rb)
//   online_commit   denoised rows -> synthesis staging, and the next state slot
//   online_istft    the offline iSTFT kernel on the synthesis staging (same pairs: the staging starts on an even frame)
//   online_emit     the final samples -> the caller
int online_push_body(nhans_online* o, const float* in, const int64_t* inoff, const int* end, float* den_out,
                     float* mix_out, const int64_t* outoff, int64_t* counts, hipStream_t s) {
    nhans_ctx* c = o->c;
    const int S = o->S;
    if (!inoff || !outoff || !counts) return fail(NHANS_EINVAL, "null argument");
    struct Plan {
        int64_t cnt, Nn, Tn, Ro, Rn, Po, Pn, lo, s0, Pend, E, nsyn;
        bool en;
    };
    std::vector<Plan> pl(S);
    int64_t tot_in = 0, tot_out = 0;
    for (int i = 0; i < S; ++i) {
        const OnStream& q = o->st[i];
        Plan& p = pl[i];
        p.cnt = inoff[i + 1] - inoff[i];
        p.en = end && end[i];
        const int rc = push_check("nhans_online_push", "stream", i, p.cnt, p.en, q.ended,
                                  o->cond[i] ? nullptr : "nhans_online_set_context / nhans_online_set_embeddings", kNoPushCap);
        if (rc) return rc;
        p.Nn = q.N + p.cnt;
        p.Tn = nhans_num_frames(p.Nn);
        if (p.Tn > kMaxFramesPerClip)
            return fail(NHANS_EINVAL, "nhans_online_push: stream " + std::to_string(i) + " would exceed " +
                                      std::to_string(kMaxFramesPerClip) + " frames");
        const int L = o->la[i];
        p.Ro = on_ready(q.T, q.ended, L); p.Po = on_paired(q.T, q.ended, L);
        p.Rn = on_ready(p.Tn, p.en || q.ended, L); p.Pn = on_paired(p.Tn, p.en || q.ended, L);
        p.lo = on_lo(p.Ro, p.Po);
        p.s0 = on_s0(p.Po);
        p.Pend = p.Pn;
        p.E = online_emit_count(o, i, p.cnt, p.en);
        p.nsyn = p.E > 0 ? p.Pend - p.s0 : 0;
        if (outoff[i + 1] - outoff[i] < p.E)
            return fail(NHANS_EINVAL, "nhans_online_push: output room of stream " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " + std::to_string(p.E) +
                                      " needed (nhans_online_out_counts)");
        tot_in += p.cnt;
        tot_out += p.E;
    }
    if (tot_in > 0 && !in) return fail(NHANS_EINVAL, "null argument: in_dev");
    if (tot_out > 0 && (!den_out || (o->mixed && !mix_out))) return fail(NHANS_EINVAL, "null argument: output buffer");

    // ---- staging layout (compact, stream after stream) ----
    std::vector<int64_t> soff(S + 1, 0), nfoff(S + 1, 0), woff(S + 1, 0), foff(S + 1, 0), yoff(S + 1, 0), ooff(S + 1, 0);
    for (int i = 0; i < S; ++i) {
        const Plan& p = pl[i];
        const OnStream& q = o->st[i];
        soff[i + 1] = soff[i] + (q.N - (int64_t)kHop * q.T) + p.cnt;
        nfoff[i + 1] = nfoff[i] + (p.Tn - q.T);
        woff[i + 1] = woff[i] + (p.Rn > p.Ro ? p.Tn - p.lo : 0);
        foff[i + 1] = foff[i] + (p.Rn - p.Ro);
        yoff[i + 1] = yoff[i] + p.nsyn;
        ooff[i + 1] = ooff[i] + (p.nsyn > 0 ? ((p.nsyn - 1) * kHop + kWin + 3) / 4 * 4 : 0);
    }
    const int64_t F = foff[S], NF = nfoff[S], WR = woff[S], Y = yoff[S];
    if (WR * kBins >= ((int64_t)1 << 31) || soff[S] >= ((int64_t)1 << 31) * 4)
        return fail(NHANS_EINVAL, "nhans_online_push: push too large for one call (split it)");
    const int64_t wf = std::min<int64_t>(c->frames_per_chunk, std::max<int64_t>(F, 1));
    const size_t nb_st = stft_blocks(soff.data(), S, 0), nb_is = istft_blocks(yoff.data(), S);
    // (every run of n floats is ceil(n / kOnlineCopyMax) pieces; a stream has at most 19 runs per push, and with the
    // sample history two more into its ring, of kCaptureSamples floats together)
    const size_t nrun_cap = (size_t)S * 32 + (size_t)(soff[S] + (WR + F + 4 * Y) * kBins + 2 * tot_out) / kOnlineCopyMax + 64 +
                            (o->ring ? (size_t)S * (2 + kCaptureSamples / kOnlineCopyMax + 1) : 0);
    size_t bytes = ws_size(soff[S], 4) + 2 * ws_size(NF * kBins, 4) + ws_size(WR * kBins, 4) + 2 * ws_size(F * kBins, 4) +
                   3 * ws_size(Y * kBins, 4) + (o->mixed ? 2 : 1) * ws_size(ooff[S], 4) + 2 * ws_size(2 * (S + 1), 8) +
                   ws_size(2 * nb_st, 4) + ws_size(2 * nb_is, 4) + ws_size(F, 4) + ws_size(nrun_cap, sizeof(OnlineCopy));
    if (F > 0) bytes += stack_ws_bytes(c, F, S, wf);
    int rc = ws_reserve(c, bytes); if (rc) return rc;
    float* wav = ws_take<float>(c, soff[S]);
    float* nlm = ws_take<float>(c, NF * kBins);
    float* nph = ws_take<float>(c, NF * kBins);
    float* win = ws_take<float>(c, WR * kBins);
    float* ctr = ws_take<float>(c, F * kBins);
    float* dnew = ws_take<float>(c, F * kBins);
    float* yden = ws_take<float>(c, Y * kBins);
    float* yph = ws_take<float>(c, Y * kBins);
    float* ylm = ws_take<float>(c, Y * kBins);
    float* tden = ws_take<float>(c, ooff[S]);
    float* tmix = o->mixed ? ws_take<float>(c, ooff[S]) : nullptr;
    int64_t* tab_st = ws_take<int64_t>(c, 2 * (S + 1));
    int64_t* tab_is = ws_take<int64_t>(c, 2 * (S + 1));
    int* blk_st = ws_take<int>(c, 2 * nb_st);
    int* blk_is = ws_take<int>(c, 2 * nb_is);
    int* rb = ws_take<int>(c, F);
    OnlineCopy* runs_dev = ws_take<OnlineCopy>(c, nrun_cap);
    StackBufs sb{};
    if (F > 0) stack_take(c, F, S, wf, &sb);

    // ---- copy runs ----
    std::vector<OnlineCopy> runs;
    auto add = [&](const float* src, float* dst, int64_t n) {
        for (int64_t k = 0; k < n; k += kOnlineCopyMax) runs.push_back({src + k, dst + k, std::min<int64_t>(kOnlineCopyMax, n - k)});
    };
    const int cur = o->cur, nxt = 1 - cur;
    // rows [a, b) of stream i's log-magnitude (ph = false) or phase: the state holds [lo, T_old), the push [T_old, T_new)
    auto add_rows = [&](int i, bool ph, int64_t a, int64_t b, float* dst) {
        const OnStream& q = o->st[i];
        const Plan& p = pl[i];
        const int64_t m = std::min(b, q.T);
        if (m > a) add(o->slot(cur, i) + (ph ? kOnPh : kOnLm) + (a - p.lo) * kBins, dst, (m - a) * kBins);
        const int64_t a2 = std::max(a, q.T);
        if (b > a2) add((ph ? nph : nlm) + (nfoff[i] + a2 - q.T) * kBins, dst + (a2 - a) * kBins, (b - a2) * kBins);
    };
    // denoised rows [a, b): the state holds [s0, R_old), the push [R_old, R_new)
    auto add_den = [&](int i, int64_t a, int64_t b, float* dst, bool from_state) {
        const Plan& p = pl[i];
        if (from_state) {
            const int64_t m = std::min(b, p.Ro);
            if (m > a) add(o->slot(cur, i) + kOnDen + (a - p.s0) * kBins, dst, (m - a) * kBins);
        } else {
            const int64_t a2 = std::max(a, p.Ro);
            if (b > a2) add(dnew + (foff[i] + a2 - p.Ro) * kBins, dst + (a2 - a) * kBins, (b - a2) * kBins);
        }
    };
    std::vector<int> bounds(1, 0);
    // ingest
    for (int i = 0; i < S; ++i) {
        const int64_t carry = o->st[i].N - (int64_t)kHop * o->st[i].T;
        add(o->slot(cur, i) + kOnSamp, wav + soff[i], carry);
        if (pl[i].cnt > 0) add(in + inoff[i], wav + soff[i] + carry, pl[i].cnt);
        if (o->ring) {
            // (the sample history: the same launch, the caller's piece -> the slot's ring)
            int64_t cr[2][3];
            const int nr = nhans_capture_plan(o->st[i].N, pl[i].cnt, &cr[0][0]);
            for (int r = 0; r < nr; ++r)
                add(in + inoff[i] + cr[r][0], o->ring + (size_t)i * kCaptureSamples + cr[r][1], cr[r][2]);
        }
    }
    bounds.push_back((int)runs.size());
    // assemble
    std::vector<int> h_clip(F), h_t(F), h_T(F), h_rb(F);
    for (int i = 0; i < S; ++i) {
        const Plan& p = pl[i];
        if (p.Rn > p.Ro) {
            add_rows(i, false, p.lo, p.Tn, win + woff[i] * kBins);
            add_rows(i, false, p.Ro, p.Rn, ctr + foff[i] * kBins);
            for (int64_t t = p.Ro; t < p.Rn; ++t) {
                const int64_t f = foff[i] + t - p.Ro;
                // (the stream as frame t sees it ends L frames after t, however many rows this push already has: the
                // rows from there on are zero rows to the window readers, WinRows, and may lie past the end of `win`)
                h_clip[f] = i; h_t[f] = (int)t; h_T[f] = (int)std::min<int64_t>(p.Tn, t + o->la[i] + 1);
                h_rb[f] = (int)(woff[i] + t - kCenter - p.lo);
            }
        }
        if (p.nsyn > 0) {
            add_rows(i, true, p.s0, p.Pend, yph + yoff[i] * kBins);
            if (o->mixed) add_rows(i, false, p.s0, p.Pend, ylm + yoff[i] * kBins);
            add_den(i, p.s0, p.Pend, yden + yoff[i] * kBins, true);
        }
    }
    bounds.push_back((int)runs.size());
    // commit: denoised rows of this push -> synthesis staging; the next slot
    for (int i = 0; i < S; ++i) {
        const Plan& p = pl[i];
        const OnStream& q = o->st[i];
        if (p.nsyn > 0) add_den(i, p.s0, p.Pend, yden + yoff[i] * kBins, false);
        float* ns = o->slot(nxt, i);
        add(wav + soff[i] + (int64_t)kHop * (p.Tn - q.T), ns + kOnSamp, p.Nn - (int64_t)kHop * p.Tn);
        const int64_t lo_n = on_lo(p.Rn, p.Pn), s0_n = on_s0(p.Pn);
        if (p.Tn - lo_n > kOnRows || p.Rn - s0_n > kOnDenRows) return fail(NHANS_EINVAL, "nhans_online_push: internal state bound");
        add_rows(i, false, lo_n, p.Tn, ns + kOnLm);
        add_rows(i, true, lo_n, p.Tn, ns + kOnPh);
        add_den(i, s0_n, p.Rn, ns + kOnDen, true);
        add_den(i, s0_n, p.Rn, ns + kOnDen, false);
    }
    bounds.push_back((int)runs.size());
    // emit
    for (int i = 0; i < S; ++i) {
        const Plan& p = pl[i];
        if (p.E <= 0) continue;
        const int64_t skip = (int64_t)kHop * (p.Po - p.s0);
        add(tden + ooff[i] + skip, den_out + outoff[i], p.E);
        if (o->mixed) add(tmix + ooff[i] + skip, mix_out + outoff[i], p.E);
    }
    bounds.push_back((int)runs.size());
    if (runs.size() > nrun_cap) return fail(NHANS_EINVAL, "nhans_online_push: internal run bound");

    // ---- launches ----
    rc = h2d(c, runs_dev, runs.data(), runs.size() * sizeof(OnlineCopy), s); if (rc) return rc;
    auto copies = [&](int k, const char* name) {
        const int n = bounds[k + 1] - bounds[k];
        if (n <= 0) return;
        Prof pr(c, s, name);
        launch_online_copy(name, runs_dev + bounds[k], n, s);
        int64_t fl = 0;
        for (int r = bounds[k]; r < bounds[k + 1]; ++r) fl += runs[r].n;
        pr.done(0, 8.0 * (double)fl);
    };
    copies(0, "online_ingest");
    // (from here on the rings hold this push's samples, whether the push completes, fails or is rewound)
    if (o->ring)
        for (int i = 0; i < S; ++i) {
            o->vlo[i] = std::max(o->vlo[i], pl[i].Nn - kCaptureSamples);
            o->whi[i] = std::max(o->whi[i], pl[i].Nn);
        }
    if (NF > 0) {
        std::vector<int64_t> fo;
        rc = stft_impl(c, wav, soff.data(), S, 0, nlm, nph, tab_st, blk_st, &fo, s, "online_stft"); if (rc) return rc;
    }
    copies(1, "online_assemble");
    if (F > 0) {
        rc = h2d(c, sb.f_clip, h_clip.data(), F * 4, s); if (rc) return rc;
        rc = h2d(c, sb.f_t, h_t.data(), F * 4, s); if (rc) return rc;
        rc = h2d(c, sb.f_T, h_T.data(), F * 4, s); if (rc) return rc;
        rc = h2d(c, rb, h_rb.data(), F * 4, s); if (rc) return rc;
        rc = mask_net_run(c, win, rb, ctr, F, S, o->emb, o->emb + (size_t)S * kEmb, nullptr, dnew, sb, wf, s);
        if (rc) return rc;
        if (launch_error_pending()) return NHANS_OK;      // (reported by the entry point; nothing below runs on it)
    }
    copies(2, "online_commit");
    if (Y > 0) {
        rc = istft_impl(c, yden, yph, yoff.data(), S, ooff.data(), tden, tab_is, blk_is, s, "online_istft"); if (rc) return rc;
        if (o->mixed) {
            // (tab_is / blk_is reused: same stream, the first launch has consumed them in order)
            rc = istft_impl(c, ylm, yph, yoff.data(), S, ooff.data(), tmix, tab_is, blk_is, s, "online_istft"); if (rc) return rc;
        }
    }
    copies(3, "online_emit");
    if (launch_error_pending()) return NHANS_OK;

    // ---- host state ----
    o->prev = o->st;
    for (int i = 0; i < S; ++i) {
        OnStream& q = o->st[i];
        counts[i] = pl[i].E;
        q.N = pl[i].Nn; q.T = pl[i].Tn; q.ended = q.ended || pl[i].en;
    }
    o->cur = nxt;
    o->can_rewind = true;
    return NHANS_OK;
}

}  // namespace

extern "C" {

int nhans_online_open(nhans_ctx* c, int nstreams, const float* ca, const int64_t* caoff, const float* cbw,
                      const int64_t* cboff, int want_mixed, void* stream, nhans_online** out) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(online_open_body(c, nstreams, ca, caoff, cbw, cboff, want_mixed, call.s, out));
}

int nhans_online_open_slots(nhans_ctx* c, int nslots, int want_mixed, void* stream, nhans_online** out) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(online_open_slots_body(c, nslots, want_mixed, call.s, out));
}

int nhans_online_restart(nhans_online* o, int slot) {
    if (!o) return fail(NHANS_EINVAL, "nhans_online_restart: null object");
    const int rc = slot_check(o->S, slot, "nhans_online_restart"); if (rc) return rc;
    online_restart_slot(o, slot);
    return NHANS_OK;
}

int nhans_online_set_context(nhans_online* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb,
                             void* stream, int64_t* first_frame_out) {
    if (!o) return fail(NHANS_EINVAL, "nhans_online_set_context: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(online_set_context_body(o, slot, ca, na, cbw, nb, call.s, first_frame_out));
}

int nhans_online_set_embeddings(nhans_online* o, int slot, const float* ea, const float* eb, void* stream,
                                int64_t* first_frame_out) {
    if (!o) return fail(NHANS_EINVAL, "nhans_online_set_embeddings: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(online_set_embeddings_body(o, slot, ea, eb, call.s, first_frame_out));
}

int nhans_online_push(nhans_online* o, const float* in, const int64_t* inoff, const int* end, float* den_out,
                      float* mix_out, const int64_t* outoff, int64_t* counts, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(online_push_body(o, in, inoff, end, den_out, mix_out, outoff, counts, call.s));
}

int nhans_online_out_counts(const nhans_online* o, const int64_t* in_counts, const int* end, int64_t* counts) {
    if (!o || !in_counts || !counts) return fail(NHANS_EINVAL, "null argument");
    for (int i = 0; i < o->S; ++i) {
        const int rc = push_check("nhans_online_out_counts", "stream", i, in_counts[i], end && end[i], o->st[i].ended, nullptr, kNoPushCap);
        if (rc) return rc;
    }
    for (int i = 0; i < o->S; ++i) counts[i] = online_emit_count(o, i, in_counts[i], end && end[i]);
    return NHANS_OK;
}

int nhans_online_set_lookahead(nhans_online* o, int slot, int lookahead) {
    if (!o) return fail(NHANS_EINVAL, "nhans_online_set_lookahead: null object");
    const int rc = slot_check(o->S, slot, "nhans_online_set_lookahead"); if (rc) return rc;
    if (lookahead < 0 || lookahead > kCenter)
        return fail(NHANS_EINVAL, "nhans_online_set_lookahead: lookahead must be in [0, " + std::to_string(kCenter) + "] frames");
    if (o->st[slot].N != 0 || o->st[slot].ended)
        return fail(NHANS_EINVAL, "nhans_online_set_lookahead: slot " + std::to_string(slot) + " has a stream under way " +
                                  "(the look-ahead is set on an open stream of 0 samples: after open or nhans_online_restart)");
    o->la[slot] = lookahead;
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_online_rewind(nhans_online* o) {
    if (!o) return fail(NHANS_EINVAL, "null object");
    if (!o->can_rewind) return fail(NHANS_EINVAL, "nhans_online_rewind: no push to undo (one rewind per push)");
    online_undo(o);
    return NHANS_OK;
}

void nhans_online_close(nhans_online* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(o->emb);
    (void)hipFree(o->state);
    if (o->ring) (void)hipFree(o->ring);
    delete o;
}

}  // extern "C"

// ---- conditioning captured from a slot's own stream (include/nhans_hip.h: nhans_capture_*) --------------------------------
namespace {
static_assert(kCaptureSamples == NHANS_CAPTURE_SAMPLES, "the ring holds the 200 context frames");

int capture_enable_body(nhans_online* o, const char* fn, hipStream_t s) {
    if (o->ring) return NHANS_OK;
    float* ring = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ring), (size_t)o->S * kCaptureSamples * 4);
    if (e != hipSuccess) return fail(NHANS_ENOMEM, std::string(fn) + ": hipMalloc failed: " + hipGetErrorString(e));
    // (no capture reads a position before a push has written it -- vlo --: the zeros only keep the memory defined)
    e = hipMemsetAsync(ring, 0, (size_t)o->S * kCaptureSamples * 4, s);
    if (e != hipSuccess) {
        (void)hipFree(ring);
        return fail(NHANS_EHIP, std::string(fn) + ": hipMemsetAsync: " + hipGetErrorString(e));
    }
    o->ring = ring;
    o->vlo.resize(o->S); o->whi.resize(o->S);
    for (int i = 0; i < o->S; ++i) o->vlo[i] = o->whi[i] = o->st[i].N;
    return NHANS_OK;
}

// n entries (slot, which): ring -> clip (capture_clip_kernel), ONE STFT over the n clips, ONE tower pass over the n
// images, then the n rows into the object -- set_context's sequence with the clips taken from the device.
int capture_context_body(nhans_online* o, const char* fn_, int n, const int* slots, const int* which, int flags,
                         hipStream_t s, int64_t* first_frame) {
    nhans_ctx* c = o->c;
    const std::string fn(fn_);
    if (!o->ring) return fail(NHANS_EINVAL, fn + ": the sample history is not enabled (nhans_capture_enable)");
    if (n < 1) return fail(NHANS_EINVAL, fn + ": n must be >= 1");
    if (!slots || !which) return fail(NHANS_EINVAL, fn + ": null argument");
    if (flags & ~NHANS_CAPTURE_NORMALISE) return fail(NHANS_EINVAL, fn + ": unknown flag");
    std::vector<char> seen((size_t)2 * o->S, 0);
    for (int k = 0; k < n; ++k) {
        const int rc = slot_check(o->S, slots[k], fn_); if (rc) return rc;
        if (which[k] != NHANS_CAPTURE_A && which[k] != NHANS_CAPTURE_B)
            return fail(NHANS_EINVAL, fn + ": entry " + std::to_string(k) + ": which must be NHANS_CAPTURE_A or NHANS_CAPTURE_B");
        char& m = seen[(size_t)which[k] * o->S + slots[k]];
        if (m) return fail(NHANS_EINVAL, fn + ": slot " + std::to_string(slots[k]) + ", side " + (which[k] ? "b" : "a") + " is named twice");
        m = 1;
    }
    for (int k = 0; k < n; ++k) {
        const int i = slots[k];
        const int64_t N = o->st[i].N, lo = N - kCaptureSamples;
        if (lo >= o->vlo[i]) continue;
        const std::string head = fn + ": slot " + std::to_string(i) + ": ";
        if (lo < 0)
            return fail(NHANS_ESHORT, head + "its stream has " + std::to_string(N) + " samples so far, " +
                                      std::to_string(kCaptureSamples) + " needed");
        if (N < o->whi[i])
            return fail(NHANS_ESHORT, head + "a push was rewound and has not been repeated yet: it wrote the sample history up to sample " +
                                      std::to_string(o->whi[i]) + ", the stream stands at " + std::to_string(N));
        return fail(NHANS_ESHORT, head + "the sample history was enabled at sample " + std::to_string(o->vlo[i]) + " of its stream: " +
                                  std::to_string(N - o->vlo[i]) + " of the " + std::to_string(kCaptureSamples) + " samples needed");
    }

    std::vector<int64_t> soff(n + 1);
    for (int k = 0; k <= n; ++k) soff[k] = (int64_t)k * kCaptureSamples;
    const size_t nb = stft_blocks(soff.data(), n, kCtxFrames);
    const size_t tb = tower_buf_floats(c);
    int rc = ws_reserve(c, ws_size((size_t)n * kCaptureSamples, 4) + ws_size((size_t)n * kCtxFrames * kBins, 4) +
                               ws_size((size_t)n * kEmb, 4) + ws_size(2 * (n + 1), 8) + ws_size(2 * nb, 4) +
                               ws_size(n, sizeof(CaptureEntry)) + 3 * ws_size(tb, 4));
    if (rc) return rc;
    float* clips = ws_take<float>(c, (size_t)n * kCaptureSamples);
    float* ctxlm = ws_take<float>(c, (size_t)n * kCtxFrames * kBins);
    float* rows = ws_take<float>(c, (size_t)n * kEmb);
    int64_t* tabs = ws_take<int64_t>(c, 2 * (n + 1));
    int* blks = ws_take<int>(c, 2 * nb);
    CaptureEntry* ent_dev = ws_take<CaptureEntry>(c, n);
    float* X = ws_take<float>(c, tb); float* A = ws_take<float>(c, tb); float* Y = ws_take<float>(c, tb);
    std::vector<CaptureEntry> ent(n);
    for (int k = 0; k < n; ++k)
        ent[k] = {o->ring + (size_t)slots[k] * kCaptureSamples, clips + (size_t)k * kCaptureSamples,
                  (int)(o->st[slots[k]].N % kCaptureSamples), flags & NHANS_CAPTURE_NORMALISE};
    rc = h2d(c, ent_dev, ent.data(), (size_t)n * sizeof(CaptureEntry), s); if (rc) return rc;
    {
        Prof pr(c, s, "capture_clip_kernel");
        launch_capture_clip(ent_dev, n, s);
        pr.done(0, ((flags & NHANS_CAPTURE_NORMALISE) ? 12.0 : 8.0) * n * kCaptureSamples);
    }
    rc = stft_impl(c, clips, soff.data(), n, kCtxFrames, ctxlm, nullptr, tabs, blks, nullptr, s); if (rc) return rc;
    // (the tower writes workspace rows, not the object's: a failure leaves every slot's conditioning as it was)
    rc = embed_impl(c, ctxlm, n, rows, X, A, Y, s); if (rc) return rc;
    if (launch_error_pending()) return NHANS_OK;          // (reported by the entry point; the slots keep their rows)
    for (int k = 0; k < n; ++k)
        HIP_TRY(hipMemcpyAsync(o->emb + ((size_t)which[k] * o->S + slots[k]) * kEmb, rows + (size_t)k * kEmb, kEmb * 4,
                               hipMemcpyDeviceToDevice, s));
    o->can_rewind = false;
    if (first_frame)
        for (int k = 0; k < n; ++k) first_frame[k] = on_ready(o->st[slots[k]].T, o->st[slots[k]].ended, o->la[slots[k]]);
    return NHANS_OK;
}

int capture_embeddings_body(const nhans_online* o, const char* fn, int slot, float* ea, float* eb, hipStream_t s) {
    const int rc = slot_check(o->S, slot, fn); if (rc) return rc;
    if (ea) HIP_TRY(hipMemcpyAsync(ea, o->emb + (size_t)slot * kEmb, kEmb * 4, hipMemcpyDeviceToDevice, s));
    if (eb) HIP_TRY(hipMemcpyAsync(eb, o->emb + (size_t)(o->S + slot) * kEmb, kEmb * 4, hipMemcpyDeviceToDevice, s));
    return NHANS_OK;
}

}  // namespace

extern "C" {

int nhans_capture_plan(int64_t n_before, int64_t count, int64_t* runs_out) {
    if (n_before < 0 || count < 0) return fail(NHANS_EINVAL, "nhans_capture_plan: negative sample count");
    if (count == 0) return 0;
    if (!runs_out) return fail(NHANS_EINVAL, "nhans_capture_plan: null argument");
    const int64_t skip = std::max<int64_t>(0, count - kCaptureSamples), len = count - skip;
    const int64_t pos = (n_before + skip) % kCaptureSamples, first = std::min(len, kCaptureSamples - pos);
    runs_out[0] = skip; runs_out[1] = pos; runs_out[2] = first;
    if (first == len) return 1;
    runs_out[3] = skip + first; runs_out[4] = 0; runs_out[5] = len - first;
    return 2;
}

int nhans_capture_enable(nhans_online* o, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_capture_enable: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(capture_enable_body(o, "nhans_capture_enable", call.s));
}

int nhans_capture_context(nhans_online* o, int n, const int* slots, const int* which, int flags, void* stream,
                          int64_t* first_frame_out) {
    if (!o) return fail(NHANS_EINVAL, "nhans_capture_context: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(capture_context_body(o, "nhans_capture_context", n, slots, which, flags, call.s, first_frame_out));
}

int nhans_capture_embeddings(const nhans_online* o, int slot, float* ea, float* eb, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_capture_embeddings: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(capture_embeddings_body(o, "nhans_capture_embeddings", slot, ea, eb, call.s));
}

}  // extern "C"

// ---- sample-rate conversion and the file front end (include/nhans_hip.h: nhans_resample*, nhans_peak_normalise) --------
namespace {

int rs_filter(const char* fn, int rate_in, int rate_out, const ResampleFilter** f) {
    *f = resample_filter(rate_in, rate_out);
    if (!*f)
        return fail(NHANS_EINVAL, std::string(fn) + ": " + std::to_string(rate_in) + " Hz -> " + std::to_string(rate_out) +
                                  " Hz is not supported (one side 16000 Hz, the other 8000, 11025, 12000, 16000, 22050, "
                                  "24000, 32000, 44100, 48000, 88200 or 96000 Hz)");
    return NHANS_OK;
}

int rs_table(nhans_ctx* c, const ResampleFilter* f, const float** tab) {
    float*& t = c->rs_tab[{f->rate_in, f->rate_out}];
    if (!t) {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t), f->tab.size() * 4));
        const hipError_t e = hipMemcpy(t, f->tab.data(), f->tab.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(t); t = nullptr;
            return fail(NHANS_EHIP, std::string("hipMemcpy of the phase table: ") + hipGetErrorString(e));
        }
    }
    *tab = t;
    return NHANS_OK;
}

size_t rs_elem(int fmt) { return fmt == kResampleInt16 ? 2 : 4; }

// THE run geometry: runs for outputs [m_begin, m_end) of one clip or stream whose n_new new samples are at src (mix: see
// ResampleRun) and follow absolute index k0, stored from dst on in elements of `elem` bytes; with hist_out also an
// empty run when there is no output, so that the carried samples follow every push that brought some
void rs_add_runs(std::vector<ResampleRun>& runs, size_t* lds, const ResampleFilter& f, const void* src, const float* mix,
                 const float* hist, char* dst, size_t elem, float* hist_out, int64_t k0, int n_new, int64_t m_begin, int64_t m_end) {
    bool first = true;
    for (int64_t m = m_begin; m < m_end || (first && hist_out); m += kResampleRun) {
        const int cnt = (int)std::max<int64_t>(0, std::min<int64_t>(kResampleRun, m_end - m));
        const int64_t t0 = m * f.M + f.half, q0 = t0 / f.L;
        const int p0 = (int)(t0 - q0 * f.L);
        runs.push_back({src, mix, hist, dst ? dst + (m - m_begin) * elem : nullptr, first ? hist_out : nullptr, (long long)k0,
                        (long long)(q0 - k0), p0, n_new, cnt});
        *lds = std::max(*lds, resample_run_lds_bytes(f, p0, cnt));
        first = false;
        if (cnt == 0) break;
    }
}

// what the kernel reads and stores (launch_resample): PCM of pcm_format -> float32, or the wet/dry mix -> PCM of pcm_format
struct RateIo {
    bool from_mix;
    int pcm_format, quantise;
    float wet;
    double factor;
    bool auto_wet = false;      // from_mix: each hop's factor comes from the runs' gain table (GainTab) instead of `wet`
    size_t in_elem() const { return from_mix ? 4 : rs_elem(pcm_format); }
    size_t out_elem() const { return from_mix ? rs_elem(pcm_format) : 4; }
};

int rs_launch(nhans_ctx* c, const char* name, const std::vector<ResampleRun>& runs, const float* tab, const ResampleFilter& f,
              const RateIo& io, size_t lds, double in_bytes, int64_t out_samples, hipStream_t s) {
    if (runs.empty()) return NHANS_OK;
    int rc = ws_reserve(c, ws_size(runs.size(), sizeof(ResampleRun))); if (rc) return rc;
    ResampleRun* runs_dev = ws_take<ResampleRun>(c, runs.size());
    rc = h2d(c, runs_dev, runs.data(), runs.size() * sizeof(ResampleRun), s); if (rc) return rc;
    Prof pr(c, s, name);
    launch_resample(name, runs_dev, (int)runs.size(), tab, f, io.from_mix, io.auto_wet, io.pcm_format, io.quantise, io.wet, io.factor, lds,
                    s);
    pr.done(2.0 * f.J * (double)out_samples, in_bytes + (double)io.out_elem() * out_samples + 4.0 * runs.size() * f.tab.size());
    return NHANS_OK;
}

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

// One push through a stage, its arguments checked by the caller: the runs of every stream (stream i brings the samples
// [inoff[i], inoff[i + 1]) of `in` -- and of `mix`, where the kernel reads the mix --), ONE launch under `kernel`, then the
// commit.  Where the launch did not go out (a return code, or launch_error_pending()) nothing is committed.  gains
// (io.auto_wet): the table the runs of each stream read their hops' factors from.
int stage_push(nhans_ctx* c, RateStage& g, const char* kernel, const RateIo& io, const void* in, const float* mix,
               const int64_t* inoff, const int* end, void* out, const int64_t* outoff, int64_t* counts, hipStream_t s,
               const GainTab* gains = nullptr) {
    std::vector<ResampleRun> runs;
    std::vector<RateStage::Span> e(g.S);
    size_t lds = 0;
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < g.S; ++i) {
        const int64_t cnt = inoff[i + 1] - inoff[i];
        e[i] = g.plan(i, cnt, end && end[i]);
        const size_t first = runs.size();
        g.add_runs(runs, &lds, i, static_cast<const char*>(in) + inoff[i] * io.in_elem(), mix ? mix + inoff[i] : nullptr,
                   out ? static_cast<char*>(out) + outoff[i] * io.out_elem() : nullptr, io.out_elem(), cnt, e[i]);
        for (size_t k = first; gains && k < runs.size(); ++k) {
            runs[k].wtab = gains->w + gains->off[i];
            runs[k].hop0 = g.st.N[i] / kHop;
        }
        tin += cnt; tout += e[i].En - e[i].Eo;
    }
    const int rc = rs_launch(c, kernel, runs, g.tab, *g.f, io, lds, (double)tin * (io.in_elem() + (mix ? 4 : 0)), tout, s);
    if (rc) return rc;
    if (launch_error_pending()) return NHANS_OK;
    for (int i = 0; i < g.S; ++i) {
        counts[i] = e[i].En - e[i].Eo;
        g.commit(i, inoff[i + 1] - inoff[i], end && end[i]);
    }
    return NHANS_OK;
}

}  // namespace

struct nhans_resampler {
    nhans_ctx* c = nullptr;
    int device = 0, in_format = 0, flags = 0;
    double denom = 0.0;             // nhans_resampler_set_peak: peak + 1e-6; 0 = outputs as they are
    RateStage g;
    RateIo io() const { return {false, in_format, flags & NHANS_RESAMPLE_QUANTISE, 0.f, denom}; }
};

namespace {

int resample_body(nhans_ctx* c, const void* in, int fmt, const int64_t* inoff, int nclips, int rate_in, int rate_out,
                  int flags, float* out, const int64_t* outoff, hipStream_t s) {
    if (!inoff || !outoff || nclips < 0) return fail(NHANS_EINVAL, "nhans_resample: null argument");
    if (fmt != kResampleInt16 && fmt != kResampleFloat32) return fail(NHANS_EINVAL, "nhans_resample: in_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32");
    if (flags & ~NHANS_RESAMPLE_QUANTISE) return fail(NHANS_EINVAL, "nhans_resample: unknown flag");
    const ResampleFilter* f = nullptr;
    int rc = rs_filter("nhans_resample", rate_in, rate_out, &f); if (rc) return rc;
    std::vector<ResampleRun> runs;
    size_t lds = 0;
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = inoff[i + 1] - inoff[i];
        if (n < 0 || n > kMaxResampleClip)
            return fail(NHANS_EINVAL, "nhans_resample: clip " + std::to_string(i) + " has " + std::to_string(n) + " samples (0 ... 2^31 - 1)");
        const int64_t no = resample_out_count(*f, n);
        if (outoff[i + 1] - outoff[i] < no)
            return fail(NHANS_EINVAL, "nhans_resample: output room of clip " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " + std::to_string(no) +
                                      " needed (nhans_resample_out_count)");
        tin += n; tout += no;
    }
    if ((tin > 0 && !in) || (tout > 0 && !out)) return fail(NHANS_EINVAL, "nhans_resample: null buffer");
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = inoff[i + 1] - inoff[i];
        rs_add_runs(runs, &lds, *f, static_cast<const char*>(in) + inoff[i] * rs_elem(fmt), nullptr, nullptr,
                    reinterpret_cast<char*>(out + outoff[i]), 4, nullptr, 0, (int)n, 0, resample_out_count(*f, n));
    }
    if (runs.empty()) return NHANS_OK;
    const float* tab = nullptr;
    rc = rs_table(c, f, &tab); if (rc) return rc;
    return rs_launch(c, "resample", runs, tab, *f, {false, fmt, flags & NHANS_RESAMPLE_QUANTISE, 0.f, 0.0}, lds,
                     (double)tin * rs_elem(fmt), tout, s);
}

int peak_normalise_body(nhans_ctx* c, const float* in, const int64_t* off, int nclips, int flags, float* out, hipStream_t s) {
    if (!off || nclips < 0) return fail(NHANS_EINVAL, "nhans_peak_normalise: null argument");
    if (flags & ~NHANS_NORMALISE_WRAP_INT16) return fail(NHANS_EINVAL, "nhans_peak_normalise: unknown flag");
    std::vector<NormBlock> blocks;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = off[i + 1] - off[i];
        if (n < 0) return fail(NHANS_EINVAL, "nhans_peak_normalise: clip " + std::to_string(i) + " has a negative sample count");
        const int64_t nb = (n + kNormBlock - 1) / kNormBlock;
        if ((int64_t)blocks.size() + nb > (int64_t)1 << 30) return fail(NHANS_EINVAL, "nhans_peak_normalise: batch too large for one call");
        const int pb0 = (int)blocks.size();
        for (int64_t b = 0; b < nb; ++b)
            blocks.push_back({(long long)(off[i] + b * kNormBlock), (int)std::min<int64_t>(kNormBlock, n - b * kNormBlock), pb0, (int)nb});
    }
    if (blocks.empty()) return NHANS_OK;
    if (!in || !out) return fail(NHANS_EINVAL, "nhans_peak_normalise: null buffer");
    int rc = ws_reserve(c, ws_size(blocks.size(), sizeof(NormBlock)) + ws_size(blocks.size(), 4)); if (rc) return rc;
    NormBlock* bd = ws_take<NormBlock>(c, blocks.size());
    float* partial = ws_take<float>(c, blocks.size());
    rc = h2d(c, bd, blocks.data(), blocks.size() * sizeof(NormBlock), s); if (rc) return rc;
    const double n = (double)(off[nclips] - off[0]);
    { Prof pr(c, s, "peak_partial"); launch_peak_partial(in, bd, (int)blocks.size(), flags & NHANS_NORMALISE_WRAP_INT16, partial, s); pr.done(0, 4.0 * n); }
    if (launch_error_pending()) return NHANS_OK;
    { Prof pr(c, s, "peak_normalise"); launch_peak_normalise(in, bd, (int)blocks.size(), partial, out, s); pr.done(0, 8.0 * n); }
    return NHANS_OK;
}

int resampler_check_push(const nhans_resampler* o, const char* fn, int i, int64_t cnt, bool en) {
    return push_check(fn, "stream", i, cnt, en, o->g.st.ended[i], nullptr, kMaxResampleClip);
}

int resampler_push_body(nhans_resampler* o, const void* in, const int64_t* inoff, const int* end, float* out,
                        const int64_t* outoff, int64_t* counts, hipStream_t s) {
    if (!inoff || !outoff || !counts) return fail(NHANS_EINVAL, "nhans_resampler_push: null argument");
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < o->g.S; ++i) {
        const int64_t cnt = inoff[i + 1] - inoff[i];
        const bool en = end && end[i];
        const int rc = resampler_check_push(o, "nhans_resampler_push", i, cnt, en); if (rc) return rc;
        const RateStage::Span e = o->g.plan(i, cnt, en);
        if (outoff[i + 1] - outoff[i] < e.En - e.Eo)
            return fail(NHANS_EINVAL, "nhans_resampler_push: output room of stream " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " + std::to_string(e.En - e.Eo) +
                                      " needed (nhans_resampler_out_counts)");
        tin += cnt; tout += e.En - e.Eo;
    }
    if ((tin > 0 && !in) || (tout > 0 && !out)) return fail(NHANS_EINVAL, "nhans_resampler_push: null buffer");
    return stage_push(o->c, o->g, "resampler_push", o->io(), in, nullptr, inoff, end, out, outoff, counts, s);
}

}  // namespace

extern "C" {

int64_t nhans_resample_out_count(int64_t n, int rate_in, int rate_out) {
    const ResampleFilter* f = nullptr;
    if (rs_filter("nhans_resample_out_count", rate_in, rate_out, &f)) return NHANS_EINVAL;
    if (n < 0) return fail(NHANS_EINVAL, "nhans_resample_out_count: negative sample count");
    return resample_out_count(*f, n);
}

int64_t nhans_resample_emitted(int64_t n, int ended, int rate_in, int rate_out) {
    const ResampleFilter* f = nullptr;
    if (rs_filter("nhans_resample_emitted", rate_in, rate_out, &f)) return NHANS_EINVAL;
    if (n < 0) return fail(NHANS_EINVAL, "nhans_resample_emitted: negative sample count");
    return resample_emitted(*f, n, ended != 0);
}

int nhans_resample_taps(int rate_in, int rate_out, double* out, int cap) {
    const ResampleFilter* f = nullptr;
    const int rc = rs_filter("nhans_resample_taps", rate_in, rate_out, &f); if (rc) return rc;
    const int n = (int)f->h.size();
    if (out) {
        if (cap < n) return fail(NHANS_EINVAL, "nhans_resample_taps: room for " + std::to_string(cap) + " taps, " + std::to_string(n) + " needed");
        std::memcpy(out, f->h.data(), (size_t)n * sizeof(double));
    }
    return n;
}

int nhans_resample(nhans_ctx* c, const void* in, int in_format, const int64_t* inoff, int nclips, int rate_in, int rate_out,
                   int flags, float* out, const int64_t* outoff, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(resample_body(c, in, in_format, inoff, nclips, rate_in, rate_out, flags, out, outoff, call.s));
}

int nhans_peak_normalise(nhans_ctx* c, const float* in, const int64_t* off, int nclips, int flags, float* out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    return call.finish(peak_normalise_body(c, in, off, nclips, flags, out, call.s));
}

int nhans_channel_mean(nhans_ctx* c, const float* in, int nchan, int64_t n, float* out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    if (nchan < 1 || n < 0 || n >= ((int64_t)1 << 39)) return call.finish(fail(NHANS_EINVAL, "nhans_channel_mean: nchannels must be >= 1 and 0 <= nsamples < 2^39"));
    if (n > 0 && (!in || !out)) return call.finish(fail(NHANS_EINVAL, "nhans_channel_mean: null buffer"));
    Prof pr(c, call.s, "channel_mean");
    launch_channel_mean(in, nchan, n, out, call.s);
    pr.done(0, 4.0 * (double)n * (nchan + 1));
    return call.finish(NHANS_OK);
}

int nhans_resampler_open(nhans_ctx* c, int nstreams, int rate_in, int rate_out, int in_format, int flags, nhans_resampler** out) {
    if (!out) return fail(NHANS_EINVAL, "nhans_resampler_open: null argument");
    *out = nullptr;
    int rc = check_ctx(c); if (rc) return rc;
    if (nstreams < 1) return fail(NHANS_EINVAL, "nhans_resampler_open: nstreams must be >= 1");
    if (in_format != kResampleInt16 && in_format != kResampleFloat32)
        return fail(NHANS_EINVAL, "nhans_resampler_open: in_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32");
    if (flags & ~NHANS_RESAMPLE_QUANTISE) return fail(NHANS_EINVAL, "nhans_resampler_open: unknown flag");
    const ResampleFilter* f = nullptr;
    rc = rs_filter("nhans_resampler_open", rate_in, rate_out, &f); if (rc) return rc;
    nhans_resampler* o = new nhans_resampler();
    o->c = c; o->device = c->device; o->in_format = in_format; o->flags = flags;
    rc = o->g.alloc(c, "nhans_resampler_open", f, nstreams);
    if (rc) { delete o; return rc; }
    *out = o;
    return NHANS_OK;
}

int nhans_resampler_set_peak(nhans_resampler* o, double peak) {
    if (!o) return fail(NHANS_EINVAL, "nhans_resampler_set_peak: null object");
    if (!(peak >= 0.0) || !std::isfinite(peak)) return fail(NHANS_EINVAL, "nhans_resampler_set_peak: the peak must be finite and >= 0");
    o->denom = peak + 0.000001;
    return NHANS_OK;
}

int nhans_resampler_push(nhans_resampler* o, const void* in, const int64_t* inoff, const int* end, float* out,
                         const int64_t* outoff, int64_t* counts, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_resampler_push: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(resampler_push_body(o, in, inoff, end, out, outoff, counts, call.s));
}

int nhans_resampler_out_counts(const nhans_resampler* o, const int64_t* in_counts, const int* end, int64_t* counts) {
    if (!o || !in_counts || !counts) return fail(NHANS_EINVAL, "nhans_resampler_out_counts: null argument");
    for (int i = 0; i < o->g.S; ++i) {
        const int rc = resampler_check_push(o, "nhans_resampler_out_counts", i, in_counts[i], end && end[i]); if (rc) return rc;
    }
    for (int i = 0; i < o->g.S; ++i) {
        const RateStage::Span e = o->g.plan(i, in_counts[i], end && end[i]);
        counts[i] = e.En - e.Eo;
    }
    return NHANS_OK;
}

int nhans_resampler_restart(nhans_resampler* o, int i) {
    if (!o) return fail(NHANS_EINVAL, "nhans_resampler_restart: null object");
    if (i < 0 || i >= o->g.S)
        return fail(NHANS_EINVAL, "nhans_resampler_restart: stream " + std::to_string(i) + " out of range (0 ... " + std::to_string(o->g.S - 1) + ")");
    o->g.restart(i);
    return NHANS_OK;
}

void nhans_resampler_close(nhans_resampler* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    o->g.release();
    delete o;
}

}  // extern "C"

// ---- live PCM sessions (include/nhans_hip.h: nhans_live_*) -----------------------------------------------------------
// One object = an incoming converter (rate_in -> 16 kHz with the fixed peak), an online object and an outgoing converter
// (16 kHz -> rate_out, fed by the wet/dry mix), with the 16 kHz pieces between them in device buffers of the object.  A
// push runs the three stages inside ONE Call on one stream; the stages' own workspace needs (run tables, the online
// staging) follow each other in the context's workspace, which stream order makes safe, and nothing a later stage reads
// lives there.

// The level meter of a live object (nhans_level_live_enable; level.hip): per slot a double-buffered state of kLevelState
// doubles -- a push reads half cur[i] and writes the other one, as RateStage::hist --, and the gain table of the last
// push, which the outgoing stage reads and which therefore is a buffer of the object, not workspace.  The hops a slot's
// stream has are those of the outgoing stage's sample count (level_hops), so the snapshot of a push is h0 and cur alone.
struct LevelMeter {
    bool on = false, auto_wet = false;
    int W = 0;                      // the window of the meter and of the automatic factor (0: cumulative)
    double wmax = 1.0;
    double* state = nullptr;        // [2][S][kLevelState]
    float* wtab = nullptr;
    size_t wtab_cap = 0;            // (floats)
    struct Slots {
        std::vector<int64_t> h0;    // the first hop of the slot's stream the state knows
        std::vector<char> cur;
    } st;
    std::vector<int64_t> woff;      // the last push's hops per slot, as offsets into wtab ([S + 1]; empty: none to read)
};

struct nhans_live {
    nhans_ctx* c = nullptr;
    int device = 0, S = 0, in_format = 0, out_format = 0;
    bool has_wet = false;           // NHANS_LIVE_WET: the online object also makes the mixed round trip
    float wet = 0.f;
    double in_denom = 0.0, out_scale = 1.0;     // the fixed peak + 1e-6
    RateStage in, out;              // out's stream is c = den + (mix - den) * wet; out.st.N: 16 kHz samples taken per slot
    nhans_online* on = nullptr;
    RateStage::Streams undo_in, undo_out;       // the converters before the last push
    float *mid = nullptr, *den = nullptr, *mix = nullptr;   // the push's 16 kHz input / denoised / mixed pieces
    size_t mid_cap = 0, out_cap = 0;                        // (floats)
    bool can_rewind = false;
    LevelMeter lv;
    LevelMeter::Slots undo_lv;
    double* lv_half(int k, int i) const { return lv.state + ((size_t)k * S + i) * kLevelState; }
};

namespace {

int live_filters(const char* fn, int rate_in, int rate_out, const ResampleFilter** fi, const ResampleFilter** fo) {
    *fi = resample_filter(rate_in, 16000);
    *fo = resample_filter(16000, rate_out);
    if (!*fi || !*fo)
        return fail(NHANS_EINVAL, std::string(fn) + ": " + std::to_string(rate_in) + " Hz in / " + std::to_string(rate_out) +
                                  " Hz out is not supported (each one of 8000, 11025, 12000, 16000, 22050, 24000, 32000, "
                                  "44100, 48000, 88200 or 96000 Hz)");
    return NHANS_OK;
}

int live_check_push(const nhans_live* o, const char* fn, int i, int64_t cnt, bool en) {
    return push_check(fn, "slot", i, cnt, en, o->in.st.ended[i],
                      o->on->cond[i] ? nullptr : "nhans_live_set_context / nhans_live_set_embeddings", kMaxResampleClip);
}

// what a push of cnt samples (en: and the end) to slot i moves between the stages: n16 samples into the online object,
// d16 final samples out of it, outputs [Eo, En) of the outgoing stream
struct LivePlan {
    int64_t n16, d16, Eo, En;
};
LivePlan live_plan(const nhans_live* o, int i, int64_t cnt, bool en) {
    LivePlan p{};
    const RateStage::Span e16 = o->in.plan(i, cnt, en);
    p.n16 = e16.En - e16.Eo;
    p.d16 = online_emit_count(o->on, i, p.n16, en);
    const RateStage::Span e = o->out.plan(i, p.d16, en);
    p.Eo = e.Eo; p.En = e.En;
    return p;
}

// Grows on demand, at least doubling: equal-sized pushes stop growing after their first few.  (hipFree waits for the
// device, so a buffer an earlier push still uses is not taken from under it.)
int live_grow(float** p, size_t want) {
    float* q = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), want * 4);
    if (e != hipSuccess) return fail(NHANS_ENOMEM, std::string("nhans_live_push: hipMalloc failed: ") + hipGetErrorString(e));
    if (*p) (void)hipFree(*p);
    *p = q;
    return NHANS_OK;
}

int live_reserve(nhans_live* o, size_t n_mid, size_t n_out) {
    if (n_mid > o->mid_cap) {
        const size_t want = std::max<size_t>({n_mid, 2 * o->mid_cap, 4096});
        const int rc = live_grow(&o->mid, want); if (rc) return rc;
        o->mid_cap = want;
    }
    if (n_out > o->out_cap) {
        const size_t want = std::max<size_t>({n_out, 2 * o->out_cap, 4096});
        // (out_cap moves last: after a failure the next push tries again)
        int rc = live_grow(&o->den, want); if (rc) return rc;
        if (o->has_wet) { rc = live_grow(&o->mix, want); if (rc) return rc; }
        o->out_cap = want;
    }
    return NHANS_OK;
}

int64_t level_hops(int64_t emitted, bool ended) { return ended ? (emitted + kHop - 1) / kHop : emitted / kHop; }

// The level launch of a push whose online stage has put the pieces [ooff) into den / mix: one run per slot with new hops,
// the gains into lv.wtab from woff[i] on, the state into the half the slot's next push will read.  Host state does not
// move here: *next is what lv.st becomes once the whole push has gone out.
int live_level(nhans_live* o, const int64_t* ooff, const int* end, hipStream_t s, std::vector<int64_t>* woff,
               LevelMeter::Slots* next) {
    nhans_ctx* c = o->c;
    LevelMeter& lv = o->lv;
    const int S = o->S;
    woff->assign(S + 1, 0);
    *next = lv.st;
    for (int i = 0; i < S; ++i) {
        const int64_t N = o->out.st.N[i];
        const bool was = o->out.st.ended[i];
        (*woff)[i + 1] = (*woff)[i] + level_hops(N + ooff[i + 1] - ooff[i], was || (end && end[i])) - level_hops(N, was);
    }
    if ((size_t)(*woff)[S] > lv.wtab_cap) {
        const size_t want = std::max<size_t>({(size_t)(*woff)[S], 2 * lv.wtab_cap, 256});
        const int rc = live_grow(&lv.wtab, want); if (rc) return rc;
        lv.wtab_cap = want;
    }
    std::vector<LevelRun> runs;
    for (int i = 0; i < S; ++i) {
        const int64_t nh = (*woff)[i + 1] - (*woff)[i];
        if (nh == 0) continue;
        const int64_t first = o->out.st.N[i] / kHop;     // (new hops: the stream had not ended, its hops were whole)
        const int k = lv.st.cur[i];
        runs.push_back({o->den + ooff[i], o->mix + ooff[i], first > lv.st.h0[i] ? o->lv_half(k, i) : nullptr, o->lv_half(1 - k, i),
                        o->lv_half(1 - k, i) + kLevelMeter, lv.wtab + (*woff)[i], (long long)(ooff[i + 1] - ooff[i]),
                        (long long)first, (long long)nh, (long long)lv.st.h0[i], lv.W, lv.wmax});
        next->cur[i] = (char)(1 - k);
    }
    if (runs.empty()) return NHANS_OK;
    int rc = ws_reserve(c, ws_size(runs.size(), sizeof(LevelRun))); if (rc) return rc;
    LevelRun* runs_dev = ws_take<LevelRun>(c, runs.size());
    rc = h2d(c, runs_dev, runs.data(), runs.size() * sizeof(LevelRun), s); if (rc) return rc;
    Prof pr(c, s, "live_level");
    launch_level("live_level", runs_dev, (int)runs.size(), s);
    pr.done(9.0 * (double)(ooff[S] - ooff[0]), 8.0 * (double)(ooff[S] - ooff[0]) + (double)runs.size() * 2 * kLevelState * 8);
    return NHANS_OK;
}

int live_push_body(nhans_live* o, const void* in, const int64_t* inoff, const int* end, void* out, const int64_t* outoff,
                   int64_t* counts, hipStream_t s) {
    if (!inoff || !outoff || !counts) return fail(NHANS_EINVAL, "nhans_live_push: null argument");
    nhans_ctx* c = o->c;
    const int S = o->S;
    std::vector<int64_t> moff(S + 1, 0), ooff(S + 1, 0);
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < S; ++i) {
        const int64_t cnt = inoff[i + 1] - inoff[i];
        const bool en = end && end[i];
        const int rc = live_check_push(o, "nhans_live_push", i, cnt, en); if (rc) return rc;
        const LivePlan p = live_plan(o, i, cnt, en);
        if (outoff[i + 1] - outoff[i] < p.En - p.Eo)
            return fail(NHANS_EINVAL, "nhans_live_push: output room of slot " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " +
                                      std::to_string(p.En - p.Eo) + " needed (nhans_live_out_counts)");
        moff[i + 1] = moff[i] + p.n16;
        ooff[i + 1] = ooff[i] + p.d16;
        tin += cnt; tout += p.En - p.Eo;
    }
    if ((tin > 0 && !in) || (tout > 0 && !out)) return fail(NHANS_EINVAL, "nhans_live_push: null buffer");
    int rc = live_reserve(o, (size_t)moff[S], (size_t)ooff[S]); if (rc) return rc;

    // ---- the three stages, the pieces [moff) and [ooff) between them: each commits its host state when its launches
    // went out, and a failure behind it puts it back (an online push undone leaves nothing for nhans_live_rewind) ----
    const RateStage::Streams was_in = o->in.save(), was_out = o->out.save();
    std::vector<int64_t> got(S, 0);
    rc = stage_push(c, o->in, "live_in", {false, o->in_format, 0, 0.f, o->in_denom}, in, nullptr, inoff, end, o->mid, moff.data(),
                    got.data(), s);
    if (rc || launch_error_pending()) return rc;          // (a launch error is reported by the entry point; no stage has committed)
    rc = online_push_body(o->on, o->mid, moff.data(), end, o->den, o->mix, ooff.data(), got.data(), s);
    if (rc || launch_error_pending()) { o->in.restore(was_in); return rc; }
    // (an object that never enabled its meter takes none of the branches below: launch for launch the push it was)
    std::vector<int64_t> woff;
    LevelMeter::Slots lv_next;
    if (o->lv.on) {
        rc = live_level(o, ooff.data(), end, s, &woff, &lv_next);
        if (rc || launch_error_pending()) { o->in.restore(was_in); online_undo(o->on); o->can_rewind = false; return rc; }
    }
    const bool auto_wet = o->lv.on && o->lv.auto_wet;
    const GainTab gains{o->lv.wtab, woff.data()};
    rc = stage_push(c, o->out, "live_out", {true, o->out_format, 0, o->wet, o->out_scale, auto_wet}, o->den,
                    auto_wet || o->wet != 0.f ? o->mix : nullptr, ooff.data(), end, out, outoff, counts, s, auto_wet ? &gains : nullptr);
    if (rc || launch_error_pending()) { o->in.restore(was_in); online_undo(o->on); o->can_rewind = false; return rc; }
    o->undo_in = was_in; o->undo_out = was_out;
    if (o->lv.on) {
        o->undo_lv = o->lv.st;
        o->lv.st = lv_next;
        o->lv.woff = woff;
    }
    o->can_rewind = true;
    return NHANS_OK;
}

void live_free(nhans_live* o) {
    if (o->on) nhans_online_close(o->on);
    o->in.release(); o->out.release();
    for (float* p : {o->mid, o->den, o->mix, o->lv.wtab})
        if (p) (void)hipFree(p);
    if (o->lv.state) (void)hipFree(o->lv.state);
    delete o;
}

}  // namespace

extern "C" {

namespace {
int64_t live_emitted(const char* fn, int64_t n, int ended, int rate_in, int rate_out, int L) {
    const ResampleFilter *fi = nullptr, *fo = nullptr;
    if (live_filters(fn, rate_in, rate_out, &fi, &fo)) return NHANS_EINVAL;
    if (n < 0) return fail(NHANS_EINVAL, std::string(fn) + ": negative sample count");
    if (L < 0 || L > kCenter) return fail(NHANS_EINVAL, std::string(fn) + ": lookahead must be in [0, " + std::to_string(kCenter) + "] frames");
    const int64_t n16 = resample_emitted(*fi, n, ended != 0);
    return resample_emitted(*fo, on_emitted(nhans_num_frames(n16), ended != 0, L), ended != 0);
}
}  // namespace

int64_t nhans_live_emitted(int64_t n, int ended, int rate_in, int rate_out) {
    return live_emitted("nhans_live_emitted", n, ended, rate_in, rate_out, kCenter);
}

int64_t nhans_lookahead_live_emitted(int64_t n, int ended, int rate_in, int rate_out, int lookahead) {
    return live_emitted("nhans_lookahead_live_emitted", n, ended, rate_in, rate_out, lookahead);
}

int nhans_lookahead_live_set(nhans_live* o, int slot, int lookahead) {
    if (!o) return fail(NHANS_EINVAL, "nhans_lookahead_live_set: null object");
    int rc = slot_check(o->S, slot, "nhans_lookahead_live_set"); if (rc) return rc;
    // (a stream of 0 samples in all three stages: the converter may hold samples the online stage has not seen yet)
    if (o->in.st.N[slot] != 0 || o->in.st.ended[slot])
        return fail(NHANS_EINVAL, "nhans_lookahead_live_set: slot " + std::to_string(slot) + " has a stream under way " +
                                  "(the look-ahead is set on an open stream of 0 samples: after open or nhans_live_restart)");
    rc = nhans_online_set_lookahead(o->on, slot, lookahead); if (rc) return rc;
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_live_open_slots(nhans_ctx* c, int nslots, int rate_in, int in_format, double peak, int rate_out, int out_format,
                          double out_scale, int flags, void* stream, nhans_live** out) {
    if (!out) return fail(NHANS_EINVAL, "nhans_live_open_slots: null argument");
    *out = nullptr;
    Call call(c, stream);
    if (call.rc) return call.rc;
    if (nslots < 1) return call.finish(fail(NHANS_EINVAL, "nhans_live_open_slots: nslots must be >= 1"));
    for (int fmt : {in_format, out_format})
        if (fmt != kResampleInt16 && fmt != kResampleFloat32)
            return call.finish(fail(NHANS_EINVAL, "nhans_live_open_slots: in_format and out_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32"));
    if (!(peak >= 0.0) || !std::isfinite(peak))
        return call.finish(fail(NHANS_EINVAL, "nhans_live_open_slots: the peak must be finite and >= 0"));
    if (!(out_scale > 0.0) || !std::isfinite(out_scale))
        return call.finish(fail(NHANS_EINVAL, "nhans_live_open_slots: out_scale must be finite and > 0"));
    if (flags & ~NHANS_LIVE_WET) return call.finish(fail(NHANS_EINVAL, "nhans_live_open_slots: unknown flag"));
    const ResampleFilter *fi = nullptr, *fo = nullptr;
    int rc = live_filters("nhans_live_open_slots", rate_in, rate_out, &fi, &fo); if (rc) return call.finish(rc);
    nhans_live* o = new nhans_live();
    o->c = c; o->device = c->device; o->S = nslots; o->in_format = in_format; o->out_format = out_format;
    o->has_wet = (flags & NHANS_LIVE_WET) != 0;
    o->in_denom = peak + 0.000001; o->out_scale = out_scale;
    rc = o->in.alloc(c, "nhans_live_open_slots", fi, nslots);
    if (!rc) rc = o->out.alloc(c, "nhans_live_open_slots", fo, nslots);
    if (!rc) rc = online_open_slots_body(c, nslots, o->has_wet, call.s, &o->on);
    if (rc) { live_free(o); return call.finish(rc); }
    *out = o;
    return call.finish(NHANS_OK);
}

int nhans_live_restart(nhans_live* o, int slot) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_restart: null object");
    const int rc = slot_check(o->S, slot, "nhans_live_restart"); if (rc) return rc;
    // (nothing is cleared on the device: streams of 0 samples read none of the carried state, in any of the stages)
    online_restart_slot(o->on, slot);
    o->in.restart(slot); o->out.restart(slot);
    if (o->lv.on) { o->lv.st.h0[slot] = 0; o->lv.woff.clear(); }     // (hop 0 reads none of the carried level state)
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_live_set_context(nhans_live* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb, void* stream,
                           int64_t* first_frame_out) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_set_context: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    int rc = slot_check(o->S, slot, "nhans_live_set_context"); if (rc) return call.finish(rc);
    if (!ca || !cbw) return call.finish(fail(NHANS_EINVAL, "nhans_live_set_context: null argument"));
    if (na < 0 || nb < 0) return call.finish(fail(NHANS_EINVAL, "nhans_live_set_context: negative sample count"));
    rc = online_set_context_body(o->on, slot, ca, na, cbw, nb, call.s, first_frame_out);
    if (!rc && !launch_error_pending()) o->can_rewind = false;
    return call.finish(rc);
}

int nhans_live_set_embeddings(nhans_live* o, int slot, const float* ea, const float* eb, void* stream, int64_t* first_frame_out) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_set_embeddings: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    int rc = slot_check(o->S, slot, "nhans_live_set_embeddings"); if (rc) return call.finish(rc);
    if (!ea || !eb) return call.finish(fail(NHANS_EINVAL, "nhans_live_set_embeddings: null argument"));
    rc = online_set_embeddings_body(o->on, slot, ea, eb, call.s, first_frame_out);
    if (!rc) o->can_rewind = false;
    return call.finish(rc);
}

int nhans_live_set_wet(nhans_live* o, double wet) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_set_wet: null object");
    if (!std::isfinite(wet)) return fail(NHANS_EINVAL, "nhans_live_set_wet: the factor must be finite");
    if ((float)wet != 0.f && !o->has_wet)
        return fail(NHANS_EINVAL, "nhans_live_set_wet: the object was opened without NHANS_LIVE_WET, only 0 can be set");
    o->wet = (float)wet;
    return NHANS_OK;
}

int nhans_live_out_counts(const nhans_live* o, const int64_t* in_counts, const int* end, int64_t* counts) {
    if (!o || !in_counts || !counts) return fail(NHANS_EINVAL, "nhans_live_out_counts: null argument");
    for (int i = 0; i < o->S; ++i) {
        const int rc = live_check_push(o, "nhans_live_out_counts", i, in_counts[i], end && end[i]); if (rc) return rc;
    }
    for (int i = 0; i < o->S; ++i) {
        const LivePlan p = live_plan(o, i, in_counts[i], end && end[i]);
        counts[i] = p.En - p.Eo;
    }
    return NHANS_OK;
}

int nhans_live_push(nhans_live* o, const void* in, const int64_t* inoff, const int* end, void* out, const int64_t* outoff,
                    int64_t* counts, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_push: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(live_push_body(o, in, inoff, end, out, outoff, counts, call.s));
}

int nhans_live_rewind(nhans_live* o) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_rewind: null object");
    if (!o->can_rewind) return fail(NHANS_EINVAL, "nhans_live_rewind: no push to undo (one rewind per push)");
    // (every stage wrote the half of its carried state that it did not read: the halves of before the push are intact)
    o->in.restore(o->undo_in);
    online_undo(o->on);
    o->out.restore(o->undo_out);
    if (o->lv.on) { o->lv.st = o->undo_lv; o->lv.woff.clear(); }
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_capture_live_enable(nhans_live* o, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_capture_live_enable: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(capture_enable_body(o->on, "nhans_capture_live_enable", call.s));
}

int nhans_capture_live_context(nhans_live* o, int n, const int* slots, const int* which, int flags, void* stream,
                               int64_t* first_frame_out) {
    if (!o) return fail(NHANS_EINVAL, "nhans_capture_live_context: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    const int rc = capture_context_body(o->on, "nhans_capture_live_context", n, slots, which, flags, call.s, first_frame_out);
    if (!rc && !launch_error_pending()) o->can_rewind = false;
    return call.finish(rc);
}

int nhans_capture_live_embeddings(const nhans_live* o, int slot, float* ea, float* eb, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_capture_live_embeddings: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    return call.finish(capture_embeddings_body(o->on, "nhans_capture_live_embeddings", slot, ea, eb, call.s));
}

// ---- level meter and automatic compensation (include/nhans_hip.h: nhans_level_*) ----
int64_t nhans_level_hops(int64_t emitted, int ended) {
    if (emitted < 0) return fail(NHANS_EINVAL, "nhans_level_hops: negative sample count");
    return level_hops(emitted, ended != 0);
}

int nhans_level_live_enable(nhans_live* o, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_level_live_enable: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    if (!o->has_wet)
        return call.finish(fail(NHANS_EINVAL, "nhans_level_live_enable: the object was opened without NHANS_LIVE_WET "
                                              "(the meter reads the mixed round trip)"));
    if (o->lv.on) return call.finish(NHANS_OK);
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->lv.state), (size_t)2 * o->S * kLevelState * sizeof(double));
    if (e != hipSuccess)
        return call.finish(fail(NHANS_ENOMEM, std::string("nhans_level_live_enable: hipMalloc failed: ") + hipGetErrorString(e)));
    // (nothing is cleared: a slot's first hop h0 reads none of the state)
    o->lv.st.h0.resize(o->S);
    for (int i = 0; i < o->S; ++i) o->lv.st.h0[i] = level_hops(o->out.st.N[i], o->out.st.ended[i]);
    o->lv.st.cur.assign(o->S, 0);
    o->lv.on = true;
    o->can_rewind = false;
    return call.finish(NHANS_OK);
}

namespace {
int level_check(const char* fn, int window_hops, int lowest, double wmax) {
    if (window_hops < lowest || window_hops > kLevelRing)
        return fail(NHANS_EINVAL, std::string(fn) + ": window_hops " + std::to_string(window_hops) + " outside [" +
                                  std::to_string(lowest) + ", " + std::to_string(kLevelRing) + "]");
    if (!(wmax >= 0.0) || !std::isfinite(wmax)) return fail(NHANS_EINVAL, std::string(fn) + ": wmax must be finite and >= 0");
    return NHANS_OK;
}
}  // namespace

int nhans_level_live_auto(nhans_live* o, int window_hops, double wmax) {
    if (!o) return fail(NHANS_EINVAL, "nhans_level_live_auto: null object");
    if (!o->lv.on) return fail(NHANS_EINVAL, "nhans_level_live_auto: the meter is not enabled (nhans_level_live_enable)");
    const int rc = level_check("nhans_level_live_auto", window_hops, -1, wmax); if (rc) return rc;
    o->lv.auto_wet = window_hops >= 0;
    if (window_hops >= 0) { o->lv.W = window_hops; o->lv.wmax = wmax; }
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_level_live_read(nhans_live* o, int slot, double* out, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_level_live_read: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    int rc = slot_check(o->S, slot, "nhans_level_live_read"); if (rc) return call.finish(rc);
    if (!out) return call.finish(fail(NHANS_EINVAL, "nhans_level_live_read: null argument"));
    if (!o->lv.on) return call.finish(fail(NHANS_EINVAL, "nhans_level_live_read: the meter is not enabled (nhans_level_live_enable)"));
    if (level_hops(o->out.st.N[slot], o->out.st.ended[slot]) <= o->lv.st.h0[slot])
        return call.finish(fail(NHANS_ESHORT, "nhans_level_live_read: slot " + std::to_string(slot) + " has no final hop yet"));
    hipError_t e = hipMemcpyAsync(out, o->lv_half(o->lv.st.cur[slot], slot) + kLevelMeter, 8 * sizeof(double), hipMemcpyDeviceToHost, call.s);
    if (e == hipSuccess) e = hipStreamSynchronize(call.s);
    if (e != hipSuccess) return call.finish(fail(NHANS_EHIP, std::string("nhans_level_live_read: ") + hipGetErrorString(e)));
    return call.finish(NHANS_OK);
}

int64_t nhans_level_live_gains(nhans_live* o, int slot, float* out, int64_t cap, void* stream) {
    if (!o) return fail(NHANS_EINVAL, "nhans_level_live_gains: null object");
    Call call(o->c, stream);
    if (call.rc) return call.rc;
    int rc = slot_check(o->S, slot, "nhans_level_live_gains"); if (rc) return call.finish(rc);
    if (!o->lv.on) return call.finish(fail(NHANS_EINVAL, "nhans_level_live_gains: the meter is not enabled (nhans_level_live_enable)"));
    const int64_t n = o->lv.woff.empty() ? 0 : o->lv.woff[slot + 1] - o->lv.woff[slot];
    if (!out || n == 0) { rc = call.finish(NHANS_OK); return rc ? rc : n; }
    if (cap < n)
        return call.finish(fail(NHANS_EINVAL, "nhans_level_live_gains: room for " + std::to_string(cap) + " gains, " +
                                              std::to_string(n) + " needed"));
    hipError_t e = hipMemcpyAsync(out, o->lv.wtab + o->lv.woff[slot], (size_t)n * sizeof(float), hipMemcpyDeviceToHost, call.s);
    if (e == hipSuccess) e = hipStreamSynchronize(call.s);
    if (e != hipSuccess) return call.finish(fail(NHANS_EHIP, std::string("nhans_level_live_gains: ") + hipGetErrorString(e)));
    rc = call.finish(NHANS_OK);
    return rc ? rc : n;
}

int nhans_level_gains(nhans_ctx* c, const float* den, const float* mix, const int64_t* off, int nclips, int window_hops,
                      double wmax, float* w_out, double* sums_out, void* stream) {
    Call call(c, stream);
    if (call.rc) return call.rc;
    if (!off || nclips < 0) return call.finish(fail(NHANS_EINVAL, "nhans_level_gains: null argument"));
    int rc = level_check("nhans_level_gains", window_hops, 0, wmax); if (rc) return call.finish(rc);
    std::vector<LevelRun> runs;
    int64_t hops = 0;
    for (int i = 0; i < nclips; ++i) {
        const int64_t n = off[i + 1] - off[i];
        if (n < 0) return call.finish(fail(NHANS_EINVAL, "nhans_level_gains: clip " + std::to_string(i) + " has a negative sample count"));
        const int64_t nh = level_hops(n, true);
        if (nh > 0 && (!den || !mix || !w_out)) return call.finish(fail(NHANS_EINVAL, "nhans_level_gains: null buffer"));
        if (nh > 0)
            runs.push_back({den + off[i], mix + off[i], nullptr, nullptr, sums_out ? sums_out + 8 * (size_t)i : nullptr, w_out + hops,
                            (long long)n, 0, (long long)nh, 0, window_hops, wmax});
        hops += nh;
    }
    if (runs.empty()) return call.finish(NHANS_OK);
    rc = ws_reserve(c, ws_size(runs.size(), sizeof(LevelRun))); if (rc) return call.finish(rc);
    LevelRun* runs_dev = ws_take<LevelRun>(c, runs.size());
    rc = h2d(c, runs_dev, runs.data(), runs.size() * sizeof(LevelRun), call.s); if (rc) return call.finish(rc);
    const double n = (double)(off[nclips] - off[0]);
    Prof pr(c, call.s, "level_gains");
    launch_level("level_gains", runs_dev, (int)runs.size(), call.s);
    pr.done(9.0 * n, 8.0 * n + 4.0 * (double)hops);
    return call.finish(NHANS_OK);
}

void nhans_live_close(nhans_live* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    live_free(o);
}

}  // extern "C"
