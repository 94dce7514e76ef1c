// The network on the host side: conv launch helpers, the embedding tower, the conditioned stack and head, the STFT /
// iSTFT block tables, and the offline entry points of include/nhans_hip.h that run them.
#include "host_internal.h"

namespace {

void same_pad(int n, int k, int s, int* out, int* before) {
    *out = (n + s - 1) / s;
    int total = std::max((*out - 1) * s + k - n, 0);
    *before = total / 2;
}

void fill_epilogue_defaults(nhans_ctx* c, ConvArgs& a) {
    a.zero = c->net.zero;
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
    g.kh0 = 0; g.KHfull = KH;
    return g;
}

void set_out_geometry(ConvArgs& a, int B, int Ho, int Wo, int N, int Nreal, int ldo, float* out) {
    a.Ho = Ho; a.Wo = Wo; a.M = B * Ho * Wo; a.N = N; a.Nreal = Nreal; a.ldo = ldo; a.out = out;
    a.oh0 = 0; a.Ho_full = Ho;
    a.fdHoWo = make_fastdiv((uint32_t)(Ho * Wo));
    a.fdWo = make_fastdiv((uint32_t)Wo);
}

// ---- the launches of one residual block:  x -> conv1 -> a1 -> conv2 (+ shortcut from x) -> out,  n images ---------------
// Written once for the embedding tower and the conditioned stack.  `w` holds what the block has (net_weights.h): a field
// the tower has no array for -- position tables, Winograd packs -- is null there.  `act` is the exponent index of a1; x
// is tensor act - 1 and out is tensor act + 1 (host_internal.h: TA, SA).  What only the stack has -- conditioning rows
// and clip map, the sliding-window source, the layouts and saturation limits of its StackPlan -- it sets on the result.
const float* unscale(const nhans_ctx* c, const ConvWeights& w) { return c->prec ? w.ws : nullptr; }

// conv1 of a block whose input is a one-channel image
DirectArgs first_conv_args(nhans_ctx* c, const ConvWeights& w, const BlockGeo& g, const float* x, float* a1, int n, int act) {
    DirectArgs d{};
    d.src = x; d.w = w.w; d.H = g.hin; d.W = g.win; d.KH = g.kh; d.KW = g.kw; d.sh = g.sh; d.sw = g.sw;
    int o; same_pad(g.hin, g.kh, g.sh, &o, &d.pt); same_pad(g.win, g.kw, g.sw, &o, &d.pl);
    d.Ho = g.hout; d.Wo = g.wout; d.M = n * g.hout * g.wout; d.out = a1;
    d.cb = w.cb; d.cb_stride = 0; d.img_clip = nullptr; d.tf = w.tf; d.tt = w.tt; d.ff = w.ff;
    d.relu = 1; d.fdHoWo = make_fastdiv(g.hout * g.wout); d.fdWo = make_fastdiv(g.wout);
    d.out_split = c->prec; d.sat = c->prec ? c->status_dev : nullptr; d.out_scale = c->down(act); d.sat_limit = kSatLimitF16;
    return d;
}
void run_first_conv(nhans_ctx* c, const DirectArgs& d, hipStream_t s) {
    Prof pr(c, s, "direct_conv64");
    launch_direct_conv64(d, s);
    pr.done(2.0 * d.M * d.KH * d.KW * 64, 0);
}

// what conv1 and conv2 share: the k x k segment over `src` (tensor in_act) and the epilogue terms of the conv's own arrays
ConvArgs block_conv_args(nhans_ctx* c, const ConvWeights& w, const BlockGeo& g, const float* src, int H, int W, int C, int sh,
                         int sw, int in_act) {
    ConvArgs a{};
    fill_epilogue_defaults(c, a);
    a.nseg = 1;
    a.seg[0] = make_seg(src, w.wpk[c->prec], H, W, C, g.kh, g.kw, sh, sw, true);
    a.cb = w.cb; a.tf = w.tf; a.tt = w.tt; a.ff = w.ff; a.idw = w.idw;
    a.ws = unscale(c, w);
    a.wino_u = w.wino_u; a.wino_ws = w.wino_ws;
    a.in_scale = c->up(in_act); a.out_scale = c->down(in_act + 1);
    return a;
}

ConvArgs conv1_args(nhans_ctx* c, const ConvWeights& w, const BlockGeo& g, const float* x, float* a1, int n, int act) {
    ConvArgs a = block_conv_args(c, w, g, x, g.hin, g.win, g.cin, g.sh, g.sw, act - 1);
    set_out_geometry(a, n, g.hout, g.wout, g.cout, g.cout, g.cout, a1);
    return a;
}

// conv2 with the block's shortcut: the one-channel image x itself; x as an identity residual; or, in a block that changes
// its channel count, the 1x1 strided `_transform` conv of x -- as extra K columns of this launch, or, where the caller
// runs it on its own (stack, Winograd form), its f32 output `apart` as a residual with weight one
ConvArgs conv2_args(nhans_ctx* c, const ConvWeights& w, const BlockGeo& g, const float* a1, const float* x, const float* apart,
                    float* out, int n, int act) {
    ConvArgs a = block_conv_args(c, w, g, a1, g.hout, g.wout, g.cout, 1, 1, act);
    if (g.cin == 1) {
        a.id_mode = 2; a.id = x; a.idH = g.hin; a.idW = g.win; a.idsh = g.sh; a.idsw = g.sw;
    } else if (g.cin == g.cout) {
        a.id_mode = 1; a.id = x; a.id_ld = g.cout; a.id_split = c->prec; a.id_scale = c->up(act - 1);
    } else if (apart) {
        a.id_mode = 1; a.id = apart; a.id_ld = g.cout; a.id_split = 0; a.idw = c->net.ones;
    } else {                            // (x and a1 share one exponent: tie_exponents())
        a.nseg = 2;
        a.seg[1] = make_seg(x, w.wpk_t[c->prec], g.hin, g.win, g.cin, 1, 1, g.sh, g.sw, false);
    }
    set_out_geometry(a, n, g.hout, g.wout, g.cout, g.cout, g.cout, out);
    return a;
}

// -> the name of the kernel variant that ran
const char* run_conv(nhans_ctx* c, const ConvArgs& a0, hipStream_t s) {
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
    if (a.Ho_full != a.Ho) {
        // a row-class launch stands for its rows of the direct convolution with the WHOLE filter (the rows it leaves out
        // multiply padding): `flops` stays on that basis and sums to the unsplit launch's, `mfma` is what was executed
        double kfull = 0;
        for (int i = 0; i < a.nseg; ++i) kfull += (double)a.seg[i].KHfull * a.seg[i].KW * a.seg[i].C;
        fl = 2.0 * (double)a.M * kfull * (double)a.Nreal;
    }
    p.done(fl, 0, name, mfma);
    return name;
}

struct RowClass { int oh0, rows, kh0, kh; };    // output rows [oh0, oh0 + rows) use the filter rows [kh0, kh0 + kh)

// ---- row classes: 3x3 / 4x4 convs on small images without the filter rows that read only padding -------------------
// Output row ho of a conv segment (input height H, filter height KH, row stride s, top padding pt) reads input rows
// ho*s - pt + kh; the filter rows kh whose input row lies outside [0, H) multiply zeros.  Consecutive output rows with the
// same range of useful kh form a class.  3 x 3, stride 1, pt 1: top (row 0, kh 1..2), interior (kh 0..2), bottom (row
// H - 1, kh 0..1).  -> number of classes, 0 if some output row has no useful filter row at all (such a conv is not
// split), -1 if `cap` is too small.  Ho = ceil(H / s), the output height of every conv of the network.
int row_classes(int H, int KH, int s, int pt, RowClass* out, int cap) {
    const int Ho = (H + s - 1) / s;
    int n = 0;
    for (int ho = 0; ho < Ho; ++ho) {
        const int hi0 = ho * s - pt;
        const int lo = std::max(0, -hi0), hi = std::min(KH, H - hi0);      // useful kh: [lo, hi)
        if (hi <= lo) return 0;
        if (n && out[n - 1].kh0 == lo && out[n - 1].kh == hi - lo) { ++out[n - 1].rows; continue; }
        if (n == cap) return -1;
        out[n++] = RowClass{ho, 1, lo, hi - lo};
    }
    return n;
}

// Which convs run as one launch per row class (option row_split = 1): those whose class launches together measured faster
// than the single launch in the per-kernel pass of one box -- keyed on the share of filter-row applications that multiply
// only padding, the one thing a class launch removes; what it adds is a tile's fixed cost (prologue + epilogue) for the
// partial tiles at the end of two more launches and two launch gaps.  profiles/rowsplit/README.md has the table.
//   convs (one chunk of 3,776 frame windows, ms)         H -> Ho  rows applied  share    single   classes
//   resblock4 3x3 stride 1 (x 3), conv_igemm_halo<128>     5 ->  5   15 -> 13    13.3 %   14.70    13.31   split
//   resblock4_1 conv1 3x3 stride 2, pointwise mode         9 ->  5   15 -> 13    13.3 %    2.54     2.27   split
//   resblock3 3x3 stride 1 (x 3), conv_igemm_halo<128>     9 ->  9   27 -> 25     7.4 %   13.91    13.56   split
//   resblock2_1 conv1 4x4 stride 2, pointwise mode        35 -> 18   72 -> 69     4.2 %    4.35     4.30   single launch (within the spread)
//   resblock3_1 conv1 3x3 stride 2, pointwise mode        18 ->  9   27 -> 26     3.7 %    2.36     2.44   single launch
// (not measured, single launch: resblock2's 4x4 stride-1 convs without their Winograd form, 5.6 %)
bool row_split_pays(const ConvSeg& g, const RowClass* rc, int n) {
    int applied = 0, rows = 0;
    for (int i = 0; i < n; ++i) { applied += rc[i].rows * rc[i].kh; rows += rc[i].rows; }
    return 100 * (rows * g.KH - applied) >= 7 * rows * g.KH;    // >= 7 % of the filter-row applications
}

// The launch `a` as one launch per row class, in row order on the same stream; false: `a` is not split (nothing was
// launched).  Split are f16x3 launches of the halo kernel or its pointwise mode with 128-channel tiles -- the kernels
// whose producer walks ConvSeg::kh0 / KHfull; eligibility is asked per class launch, and a class launch that came out on
// another kernel after all is an error, not a fallback.
constexpr int kMaxRowClasses = 8;
bool halo_family(ConvArgs a) {          // (launch_conv_igemm()'s order of tests, 128-channel tiles)
    if (a.variant < 2 || a.kgroup != 0 || a.N % 128 != 0 || a.in_f32 || conv_wino_eligible(a)) return false;
    a.halo64_tile512 = 0;
    return conv_igemm_halo_eligible(a) || conv_igemm_halo_pw_eligible(a);
}
bool run_conv_row_classes(nhans_ctx* c, const ConvArgs& a, hipStream_t s) {
    const ConvSeg& g = a.seg[0];
    if (!c->row_split || a.prec != 1 || a.Ho_full != a.Ho || a.M % (a.Ho * a.Wo) != 0 || !halo_family(a)) return false;
    if (a.nseg > 1 && a.seg[1].KH != 1) return false;
    RowClass rc[kMaxRowClasses];
    const int n = row_classes(g.H, g.KH, g.sh, g.pt, rc, kMaxRowClasses);
    if (n < 2 || (g.H + g.sh - 1) / g.sh != a.Ho) return false;
    if (c->row_split == 1 && !row_split_pays(g, rc, n)) return false;
    const int B = a.M / (a.Ho * a.Wo);
    ConvArgs q[kMaxRowClasses];
    for (int i = 0; i < n; ++i) {
        q[i] = a;
        q[i].Ho = rc[i].rows; q[i].M = B * rc[i].rows * a.Wo; q[i].oh0 = rc[i].oh0; q[i].Ho_full = a.Ho;
        q[i].fdHoWo = make_fastdiv((uint32_t)(rc[i].rows * a.Wo));
        ConvSeg& h = q[i].seg[0];
        h.KH = rc[i].kh; h.kh0 = rc[i].kh0; h.KHfull = g.KH; h.pt = g.pt - rc[i].kh0 - rc[i].oh0 * g.sh;
        h.nchunks = h.KH * h.KW * h.C / 32;
        if (a.nseg > 1) {               // the 1x1 strided `_transform` segment: its one filter row, from the class's first row on
            ConvSeg& t = q[i].seg[1];
            if ((rc[i].oh0 + rc[i].rows - 1) * t.sh - t.pt >= t.H || rc[i].oh0 * t.sh - t.pt < 0) return false;
            t.pt -= rc[i].oh0 * t.sh;
        }
        q[i].wino_u = nullptr; q[i].wino_ws = nullptr;      // (a class has no Winograd form)
        if (!halo_family(q[i])) return false;
    }
    for (int i = 0; i < n && !launch_error_pending(); ++i)
        if (std::strncmp(run_conv(c, q[i], s), "conv_igemm_halo", 15) != 0)
            note_refusal("row-class conv launch on a kernel that does not walk filter-row classes");
    return true;
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

size_t stack_buf_floats(const nhans_ctx* c, int64_t wf) {
    size_t m = 0;
    for (const auto& g : c->stack) m = std::max(m, (size_t)g.hout * g.wout * g.cout);
    return m * (size_t)wf;
}

// floats per frame window of StackBufs::T: the largest conv2 output among the channel-changing blocks whose conv2
// has a Winograd form (4x4 filters: resblock2_1)
size_t transform_buf_floats(const nhans_ctx* c, int64_t wf) {
    size_t m = 0;
    for (const auto& g : c->stack)
        if (g.cin != g.cout && g.cin > 1 && g.kh == 4) m = std::max(m, (size_t)g.hout * g.wout * g.cout);
    return m * (size_t)wf;
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
        if (!w && run_conv_row_classes(c, a, s)) return;
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
        const BlockWeights& w = c->net.stack[b];
        const int act = SA(b, 0);
        const float* cb1 = sb.cb_all + c->cond_off[2 * b];
        const float* cb2 = sb.cb_all + c->cond_off[2 * b + 1];
        const float* in = b ? x : lm_chunk;     // (block 0: the window image itself)
        if (b == 0) {
            DirectArgs d = first_conv_args(c, w.c1, g, in, a1, n, act);
            d.win = win; d.cb = cb1; d.cb_stride = c->cond_cols; d.img_clip = clipmap;
            d.out_split = c->prec && !stored_f32(c, plan, 0, 0); d.sat_limit = sat_limit_for(plan, 0, 2);
            if (go && !dead()) run_first_conv(c, d, s);
        } else {
            ConvArgs a = conv1_args(c, w.c1, g, in, a1, n, act);
            a.cb = cb1; a.cb_stride = c->cond_cols; a.img_clip = clipmap;
            a.sat_limit = sat_limit_for(plan, b, 2);
            a.in_f32 = stored_f32(c, plan, b - 1, 1); a.out_split = c->prec && !stored_f32(c, plan, b, 0);
            conv(b, 1, a);
        }
        if (go) tap(c, act, a1, (size_t)n * g.hout * g.wout * g.cout, g.cout, s, stored_f32(c, plan, b, 0));
        auto conv2 = [&](const float* apart, float* to) {
            ConvArgs a = conv2_args(c, w.c2, g, a1, in, apart, to, n, act);
            a.cb = cb2; a.cb_stride = c->cond_cols; a.img_clip = clipmap;
            a.sat_limit = sat_limit_for(plan, b + 1, 1);
            a.in_f32 = stored_f32(c, plan, b, 0); a.out_split = c->prec && !stored_f32(c, plan, b, 1);
            return a;
        };
        ConvArgs a;
        float* out;
        if (b == 0) {                       // 1 -> 64 transform on the window image itself
            out = x;
            a = conv2(nullptr, out);
            a.id_win = win;
        } else if (g.cin == g.cout) {       // identity shortcut, written in place over the block input
            // (in place only if input and output share a layout: a thread's output bytes are its residual bytes then)
            out = stored_f32(c, plan, b - 1, 1) == stored_f32(c, plan, b, 1) ? x : y;
            a = conv2(nullptr, out);
            a.id_split = c->prec && !stored_f32(c, plan, b - 1, 1);
        } else {
            // Channel-changing block.  If its conv2 -- as a one-segment conv with an f32 residual tensor -- has a
            // Winograd form, the 1x1 strided `_transform` conv (which cannot ride in the K loop of the transformed
            // domain; 3 % of the block's MACs) runs first on its own into an f32 tensor that conv2's epilogue then adds
            // like a residual (the bias of both is in conv2's bias row).  Otherwise it is extra K columns of conv2.
            out = y;
            a = conv2(sb.T, out);
            if (go ? plan.wino[b][2] : wino_form(a)) {
                ConvArgs t{};
                fill_epilogue_defaults(c, t);
                t.nseg = 1;
                t.seg[0] = make_seg(x, w.c2.wpk_t[c->prec], g.hin, g.win, g.cin, 1, 1, g.sh, g.sw, false);
                set_out_geometry(t, n, g.hout, g.wout, g.cout, g.cout, g.cout, sb.T);
                t.cb = c->net.zero; t.cb_stride = 0;
                t.ws = unscale(c, w.c2);            // (conv2 and the transform share one column scale: fold.py emit())
                t.relu = 0; t.out_split = 0;
                t.in_scale = c->up(act - 1);        // (f32 output: no exponent)
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
            } else {
                a = conv2(nullptr, out);
            }
        }
        conv(b, 2, a);
        if (go) tap(c, act + 1, out, (size_t)n * g.hout * g.wout * g.cout, g.cout, s, stored_f32(c, plan, b, 1));
        if (out == y) std::swap(x, y);
    }
    result = x;
    if (upto >= 9 && go && !dead()) {       // last_conv [5,1] VALID + BN + ReLU  (SN/main.py:232-236)
        const BlockGeo& g = c->stack[7];
        ConvArgs a{};
        fill_epilogue_defaults(c, a);
        a.nseg = 1;
        a.seg[0] = make_seg(x, c->net.head_conv.wpk[c->prec], g.hout, g.wout, g.cout, g.hout, 1, 1, 1, false);
        set_out_geometry(a, n, 1, g.wout, 512, 512, 512, a1);
        a.cb = c->net.head_conv.cb;
        a.ws = unscale(c, c->net.head_conv);
        a.in_scale = c->up(SA(7, 1)); a.out_scale = c->down(kActHead);
        run_conv(c, a, s);
        tap(c, kActHead, a1, (size_t)n * g.wout * 512, 512, s);
        result = a1;
    }
    }
    c->last_plan = plan;
    return result;
}

}  // namespace

// ---- embedding tower for `n` context images already in HBM ----------------------------------
int embed_impl(nhans_ctx* c, const float* ctx_lm, int n, float* emb_out, const TowerBufs& tb, hipStream_t s) {
    const auto& T = c->tower;
    for (int i0 = 0; i0 < n; i0 += c->contexts_per_chunk) {
        const int nc = std::min(c->contexts_per_chunk, n - i0);
        const float* img = ctx_lm + (size_t)i0 * kCtxFrames * kBins;
        float *x = tb.X, *a1 = tb.A, *y = tb.Y;
        for (int b = 0; b < 4; ++b) {
            const BlockGeo& g = T[b];
            const BlockWeights& w = c->net.tower[b];
            const int act = TA(b, 0);
            const float* in = b ? x : img;
            if (b == 0) {
                run_first_conv(c, first_conv_args(c, w.c1, g, in, a1, nc, act), s);
            } else {
                ConvArgs a = conv1_args(c, w.c1, g, in, a1, nc, act);
                a.kgroup = -1;                  // a handful of context images: grouped sum, split-K when small
                run_conv(c, a, s);
            }
            tap(c, act, a1, (size_t)nc * g.hout * g.wout * g.cout, g.cout, s);
            // (the `_transform` segment reads x, whose exponent tie_exponents() keeps equal to a1's: one accumulator)
            run_conv(c, conv2_args(c, w.c2, g, a1, in, nullptr, y, nc, act), s);     // (stride 1: halo kernel; measured faster than split-K here)
            tap(c, act + 1, y, (size_t)nc * g.hout * g.wout * g.cout, g.cout, s);
            std::swap(x, y);
        }
        const BlockGeo& g = T[3];
        Prof pr(c, s, "avgpool");
        launch_avgpool(x, nc, g.hout * g.wout, g.cout, c->prec, c->up(TA(3, 1)), emb_out + (size_t)i0 * kEmb, s);
        pr.done(0, (double)nc * g.hout * g.wout * g.cout * 4);
    }
    return NHANS_OK;
}

static size_t tower_buf_floats(const nhans_ctx* c) {
    size_t m = 0;
    for (const auto& g : c->tower) m = std::max(m, (size_t)g.hout * g.wout * g.cout);
    return m * (size_t)c->contexts_per_chunk;
}

void tower_plan(WsPlan& p, const nhans_ctx* c, TowerBufs* tb) {
    const size_t nb = tower_buf_floats(c);
    p.add(&tb->X, nb); p.add(&tb->A, nb); p.add(&tb->Y, nb);
}

// ---- conditioned stack + head ---------------------------------------------------------------
void stack_plan(WsPlan& p, const nhans_ctx* c, int64_t total, int nclips, int64_t wf, StackBufs* sb) {
    p.add(&sb->f_clip, total); p.add(&sb->f_t, total); p.add(&sb->f_T, total);
    p.add(&sb->foff_dev, nclips + 1);
    p.add(&sb->cb_all, (size_t)nclips * c->cond_cols);
    const size_t nb = stack_buf_floats(c, wf);
    p.add(&sb->X, nb); p.add(&sb->A, nb); p.add(&sb->Y, nb);
    p.add(&sb->T, transform_buf_floats(c, wf));
}

// The conditioning rows of `nclips` clips (production: under the profiling bracket `cond_proj`; the debug captures are not
// profiled).
static void cond_rows(nhans_ctx* c, const float* ea, const float* eb, int nclips, const StackBufs& sb, bool production, hipStream_t s) {
    if (!production) { launch_cond(ea, eb, nclips, c->net.cond_w, c->net.cond_base, c->cond_cols, sb.cb_all, s); return; }
    Prof pr(c, s, "cond_proj");
    launch_cond(ea, eb, nclips, c->net.cond_w, c->net.cond_base, c->cond_cols, sb.cb_all, s);
    pr.done(2.0 * nclips * 2 * kEmb * c->cond_cols, 0);
}

// What a run of the stack over a batch of clips (frame offsets foff) starts with: the stack's buffers for passes of wf
// frame windows placed -- commit: as the call's only scratch; otherwise the caller's own committed plan holds sb already
// --, the frame offsets on the device, the per-frame tables and the conditioning rows.
static int stack_begin(nhans_ctx* c, bool commit, const int64_t* foff, int nclips, int64_t wf, const float* ea, const float* eb,
                       bool production, StackBufs* sb, hipStream_t s) {
    const int64_t total = foff[nclips];
    int rc = NHANS_OK;
    if (commit) {
        WsPlan p;
        stack_plan(p, c, total, nclips, wf, sb);
        rc = ws_commit(c, p); if (rc) return rc;
    }
    rc = h2d(c, sb->foff_dev, foff, (nclips + 1) * sizeof(int64_t), s); if (rc) return rc;
    launch_frame_index(sb->foff_dev, nclips, total, c->lookahead, sb->f_clip, sb->f_t, sb->f_T, s);
    cond_rows(c, ea, eb, nclips, *sb, production, s);
    return NHANS_OK;
}

// The stack + head over `total` frame windows whose per-frame tables (sb.f_clip, f_t, f_T) and conditioning rows are in
// place.  win_src / rb: the window source (rb nullable, see run_stack_chunk); centre [total, 201]: the frames' own rows, the
// head's identity term (mixed_central, SN/main.py:242) -- offline that is win_src itself.
static int stack_and_head(nhans_ctx* c, const float* win_src, const int* rb, const float* centre, int64_t total, float* logits,
                          float* denoised, const StackBufs& sb, int64_t wf, hipStream_t s) {
    const BlockGeo& g = c->stack[7];
    for (int64_t g0 = 0; g0 < total; g0 += wf) {
        const int n = (int)std::min<int64_t>(wf, total - g0);
        float* hc = run_stack_chunk(c, win_src, rb, sb, g0, n, 9, s);
        if (launch_error_pending()) break;      // (reported by the entry point: NHANS_EHIP naming the launch)
        // last_dense 13312 -> 201 (+bias) and denoised = mixed_central + out  (SN/main.py:237-242)
        ConvArgs a{};
        fill_epilogue_defaults(c, a);
        a.nseg = 1;
        a.seg[0] = make_seg(hc, c->net.head_dense.wpk[c->prec], 1, 1, g.wout * 512, 1, 1, 1, 1, false);
        set_out_geometry(a, n, 1, 1, 256, kBins, kBins, denoised + g0 * kBins);
        a.cb = c->net.head_dense.cb;
        a.ws = unscale(c, c->net.head_dense);
        a.out_split = 0;
        a.relu = 0;
        a.in_scale = c->up(kActHead);
        a.id_mode = 1; a.id = centre + g0 * kBins; a.id_ld = kBins; a.idw = c->net.ones;
        if (logits) { a.aux = logits + g0 * kBins; a.aux_ld = kBins; }
        a.kgroup = -1;                          // K = 13312 over a few hundred frames: grouped sum, split-K when small
        run_conv(c, a, s);
    }
    return NHANS_OK;
}

// (online enhancement: the per-frame tables come from the object's streams, host_online.hip)
int mask_net_run(nhans_ctx* c, const float* win_src, const int* rb, const float* centre, int64_t total, int nclips,
                 const float* ea, const float* eb, float* logits, float* denoised, const StackBufs& sb, int64_t wf,
                 hipStream_t s) {
    cond_rows(c, ea, eb, nclips, sb, true, s);
    return stack_and_head(c, win_src, rb, centre, total, logits, denoised, sb, wf, s);
}

// the offline mask net over a batch of clips (commit: see stack_begin)
static int mask_net_impl(nhans_ctx* c, bool commit, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                         const float* eb, float* logits, float* denoised, StackBufs* sb, int64_t wf, hipStream_t s) {
    const int rc = stack_begin(c, commit, foff, nclips, wf, ea, eb, true, sb, s); if (rc) return rc;
    return stack_and_head(c, logmag, nullptr, logmag, foff[nclips], logits, denoised, *sb, wf, s);
}

// ---- STFT / iSTFT host-side block tables ----------------------------------------------------
int stft_impl(nhans_ctx* c, const float* wav, const int64_t* soff, int nclips, int maxf, float* logmag,
              float* phase, int64_t* dev_tables /*3*(nclips+1)*/, int* dev_blocks, std::vector<int64_t>* foff_out,
              hipStream_t s, const char* prof_name) {
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
    rc = h2d(c, dev_tables + (nclips + 1), foff, s); if (rc) return rc;
    rc = h2d(c, dev_blocks, bclip, s); if (rc) return rc;
    rc = h2d(c, dev_blocks + nb, bf0, s); if (rc) return rc;
    ClipTable t{dev_tables, dev_tables + (nclips + 1), nullptr};
    Prof pr(c, s, prof_name ? prof_name : phase ? "stft_features" : "stft_context_features");   // (contexts: log-magnitude only, 200 frames per clip)
    launch_stft(wav, t, dev_blocks, dev_blocks + nb, nb, c->net.tw400, c->net.window, logmag, phase, s);
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
               const char* prof_name) {
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
    rc = h2d(c, dev_blocks, bclip, s); if (rc) return rc;
    rc = h2d(c, dev_blocks + nb, bh0, s); if (rc) return rc;
    ClipTable t{nullptr, dev_tables, dev_tables + (nclips + 1)};
    Prof pr(c, s, prof_name);
    launch_istft(logmag, phase, t, dev_blocks, dev_blocks + nb, nb, c->net.tw400, c->net.wsyn, wav_out, s);
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

// ---- the whole offline path (nhans_enhance_clips; the built-in calibration of nhans_create: host_ctx.hip) ---------
int enhance_clips_body(nhans_ctx* c, const float* mix, const int64_t* moff, int nclips, const float* ca,
                        const int64_t* caoff, const float* cbw, const int64_t* cboff, float* den_wav,
                        float* mixed_wav, float* logmag_out, float* phase_out, float* logits_out, float* emb_out,
                        hipStream_t s) {
    int rc = NHANS_OK;
    if (!mix || !moff || !ca || !caoff || !cbw || !cboff || !den_wav || nclips < 1)
        return fail(NHANS_EINVAL, "null argument");
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
    WsPlan p;
    float *lm, *ph, *den, *lg, *ctxlm, *emb;
    int64_t* tabs[4]; int* blks[4];
    TowerBufs tb; StackBufs sb;
    p.add(&lm, (size_t)total * kBins);
    p.add(&ph, (size_t)total * kBins);
    p.add(&den, (size_t)total * kBins);
    p.add(&lg, (size_t)total * kBins);
    p.add(&ctxlm, (size_t)2 * nclips * kCtxFrames * kBins);
    p.add(&emb, (size_t)2 * nclips * kEmb);
    for (int i = 0; i < 4; ++i) { p.add(&tabs[i], 2 * (nclips + 1)); p.add(&blks[i], 2 * nblk); }
    // (the tower is done with its buffers before the stack's first launch, on the same stream: the two share their place)
    const size_t shared = p.mark();
    tower_plan(p, c, &tb);
    p.rewind(shared);
    stack_plan(p, c, total, nclips, wf, &sb);
    // option phase_iters: the refinement's planes share that place too (the stack is done with its buffers by then), and its
    // result is a plane of its own -- the phase_out_dev tap and the mixed_wav round trip keep the mixture's phase
    const bool refine = c->phase_iters > 0 && total > 0;
    PhaseBufs pb; float* ph_ref = nullptr;
    if (refine) {
        p.rewind(shared);
        p.add(&ph_ref, (size_t)total * kBins);
        phase_plan(p, foff.data(), nclips, c->phase_alpha != 0.0, &pb);
    }
    rc = ws_commit(c, p); if (rc) return rc;

    rc = stft_impl(c, mix, moff, nclips, 0, lm, ph, tabs[0], blks[0], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, ca, caoff, nclips, kCtxFrames, ctxlm, nullptr, tabs[1], blks[1], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, cbw, cboff, nclips, kCtxFrames, ctxlm + (size_t)nclips * kCtxFrames * kBins, nullptr, tabs[2],
                   blks[2], nullptr, s);
    if (rc) return rc;
    rc = embed_impl(c, ctxlm, 2 * nclips, emb, tb, s); if (rc) return rc;
    if (total > 0) {
        rc = mask_net_impl(c, false, lm, foff.data(), nclips, emb, emb + (size_t)nclips * kEmb, lg, den, &sb, wf, s);
        if (rc) return rc;
        if (refine) {
            rc = phase_refine_run(c, den, ph, foff.data(), nclips, c->phase_iters, c->phase_alpha, ph_ref, nullptr, pb, s);
            if (rc) return rc;
        }
        rc = istft_impl(c, den, refine ? ph_ref : ph, foff.data(), nclips, moff, den_wav, tabs[3], blks[3], s); if (rc) return rc;
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

// ================================================================================================
extern "C" {

size_t nhans_workspace_bytes(nhans_ctx* c, int64_t total_frames, int nclips) {
    if (!c) return 0;
    const int64_t wf = std::min<int64_t>(c->frames_per_chunk, std::max<int64_t>(total_frames, 1));
    // an uncommitted plan, for its size alone: enhance_clips_body's without its small tables -- the rows and the
    // conditioning, then tower and stack in one place
    WsPlan p; StackBufs sb; TowerBufs tb; float* f;
    for (int i = 0; i < 4; ++i) p.add(&f, (size_t)total_frames * kBins);    // logmag, phase, denoised, logits
    p.add(&f, (size_t)2 * nclips * kCtxFrames * kBins);
    p.add(&f, (size_t)2 * nclips * kEmb);
    const size_t shared = p.mark();
    tower_plan(p, c, &tb);
    p.rewind(shared);
    stack_plan(p, c, total_frames, nclips, wf, &sb);
    return p.bytes() + (1 << 20);
}

int nhans_stft_features(nhans_ctx* c, const float* wav, const int64_t* soff, int nclips, int maxf,
                        float* logmag, float* phase, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!wav || !soff || !logmag || nclips < 0) return fail(NHANS_EINVAL, "null argument");
        const size_t nb = stft_blocks(soff, nclips, maxf);
        WsPlan p;
        int64_t* tabs; int* blocks;
        p.add(&tabs, 2 * (nclips + 1)); p.add(&blocks, 2 * nb);
        const int rc = ws_commit(c, p); if (rc) return rc;
        return stft_impl(c, wav, soff, nclips, maxf, logmag, phase, tabs, blocks, nullptr, s);
    });
}

int nhans_embed(nhans_ctx* c, const float* ctx_lm, int n, float* emb_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!ctx_lm || !emb_out || n < 0) return fail(NHANS_EINVAL, "null argument");
        WsPlan p; TowerBufs tb;
        tower_plan(p, c, &tb);
        const int rc = ws_commit(c, p); if (rc) return rc;
        return embed_impl(c, ctx_lm, n, emb_out, tb, s);
    });
}

int nhans_mask_net(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                   const float* eb, float* logits, float* denoised, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!logmag || !foff || !ea || !eb || !denoised || nclips < 1) return fail(NHANS_EINVAL, "null argument");
        const int64_t total = foff[nclips];
        if (total <= 0) return NHANS_OK;
        StackBufs sb;
        return mask_net_impl(c, true, logmag, foff, nclips, ea, eb, logits, denoised, &sb, std::min<int64_t>(c->frames_per_chunk, total), s);
    });
}

int nhans_debug_row_classes(int H, int KH, int stride, int pt, int* out, int cap) {
    if (H < 1 || KH < 1 || stride < 1 || pt < 0 || cap < 0 || (cap && !out)) return fail(NHANS_EINVAL, "row classes: bad argument");
    std::vector<RowClass> rc((size_t)(H + stride - 1) / stride);
    const int n = row_classes(H, KH, stride, pt, rc.data(), (int)rc.size());
    if (n > cap) return fail(NHANS_EINVAL, "row classes: " + std::to_string(n) + " classes, room for " + std::to_string(cap));
    for (int i = 0; i < n; ++i) { out[4 * i] = rc[i].oh0; out[4 * i + 1] = rc[i].rows; out[4 * i + 2] = rc[i].kh0; out[4 * i + 3] = rc[i].kh; }
    return n;
}

int nhans_debug_block_output(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                             const float* eb, int64_t frame0, int nframes, int block, float* out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!logmag || !foff || !ea || !eb || !out || block < 0 || block > 8) return fail(NHANS_EINVAL, "bad argument");
        if (frame0 < 0 || frame0 + nframes > foff[nclips]) return fail(NHANS_EINVAL, "frame range outside batch");
        StackBufs sb;
        const int rc = stack_begin(c, true, foff, nclips, nframes, ea, eb, false, &sb, s); if (rc) return rc;
        const float* res = run_stack_chunk(c, logmag, nullptr, sb, frame0, nframes, block + 1, s);
        size_t per;
        if (block == 8) per = (size_t)26 * 512;
        else per = (size_t)c->stack[block].hout * c->stack[block].wout * c->stack[block].cout;
        if (c->prec && block < 8 && stored_f32(c, c->last_plan, block, 1)) launch_scale_copy(res, per * nframes, c->up(SA(block, 1)), out, s);
        else if (c->prec) launch_unsplit(res, (int64_t)nframes * (int64_t)(per / (block == 8 ? 512 : c->stack[block].cout)),
                                    block == 8 ? 512 : c->stack[block].cout, c->up(block == 8 ? kActHead : SA(block, 1)), out, s);
        else HIP_TRY(hipMemcpyAsync(out, res, per * nframes * 4, hipMemcpyDeviceToDevice, s));
        return NHANS_OK;
    });
}

// Any stored tensor of the stack + head (index 8 .. 24) for frames [frame0, frame0 + nframes): the production launch
// sequence -- one plan for the whole stack, frames_per_chunk frame windows per pass counted from frame0 -- up to the block
// that writes it; the tap() point of that tensor converts every chunk's finished buffer.
int nhans_debug_activation(nhans_ctx* c, const float* logmag, const int64_t* foff, int nclips, const float* ea,
                           const float* eb, int64_t frame0, int nframes, int index, float* out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!logmag || !foff || !ea || !eb || !out || nclips < 1 || nframes < 1) return fail(NHANS_EINVAL, "bad argument");
        if (index < SA(0, 0) || index >= kNumAct)
            return fail(NHANS_EINVAL, "activation index outside the stack's 8 .. " + std::to_string(kNumAct - 1) + " (tower tensors: nhans_debug_tower_activation)");
        if (frame0 < 0 || frame0 + nframes > foff[nclips]) return fail(NHANS_EINVAL, "frame range outside batch");
        const int64_t wf = std::min<int64_t>(c->frames_per_chunk, nframes);
        StackBufs sb;
        const int rc = stack_begin(c, true, foff, nclips, wf, ea, eb, false, &sb, s); if (rc) return rc;
        const int upto = index == kActHead ? 9 : (index - SA(0, 0)) / 2 + 1;
        c->cap_idx = index; c->cap_out = out;
        for (int64_t g0 = frame0; g0 < frame0 + nframes; g0 += wf) {
            run_stack_chunk(c, logmag, nullptr, sb, g0, (int)std::min<int64_t>(wf, frame0 + nframes - g0), upto, s);
            if (launch_error_pending()) break;
        }
        c->cap_idx = -1; c->cap_out = nullptr;
        return NHANS_OK;
    });
}

// Any stored tensor of the embedding tower (index 0 .. 7) for n context images: nhans_embed's own launches (chunks of
// contexts_per_chunk images, the pooled embeddings go to the workspace) with the tap() point of that tensor copying out.
int nhans_debug_tower_activation(nhans_ctx* c, const float* ctx_lm, int n, int index, float* out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!ctx_lm || !out || n < 1) return fail(NHANS_EINVAL, "bad argument");
        if (index < 0 || index >= SA(0, 0))
            return fail(NHANS_EINVAL, "activation index outside the tower's 0 .. 7 (stack tensors: nhans_debug_activation)");
        WsPlan p; TowerBufs tb; float* emb;
        tower_plan(p, c, &tb);
        p.add(&emb, (size_t)n * kEmb);
        int rc = ws_commit(c, p); if (rc) return rc;
        c->cap_idx = index; c->cap_out = out;
        rc = embed_impl(c, ctx_lm, n, emb, tb, s);
        c->cap_idx = -1; c->cap_out = nullptr;
        return rc;
    });
}

int nhans_istft(nhans_ctx* c, const float* logmag, const float* phase, const int64_t* foff, int nclips,
                const int64_t* ooff, float* wav_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!logmag || !phase || !foff || !ooff || !wav_out) return fail(NHANS_EINVAL, "null argument");
        const size_t nb = istft_blocks(foff, nclips);
        WsPlan p;
        int64_t* tabs; int* blocks;
        p.add(&tabs, 2 * (nclips + 1)); p.add(&blocks, 2 * nb);
        const int rc = ws_commit(c, p); if (rc) return rc;
        return istft_impl(c, logmag, phase, foff, nclips, ooff, wav_out, tabs, blocks, s);
    });
}

int nhans_enhance_clips(nhans_ctx* c, const float* mix, const int64_t* moff, int nclips, const float* ca,
                        const int64_t* caoff, const float* cbw, const int64_t* cboff, float* den_wav,
                        float* mixed_wav, float* logmag_out, float* phase_out, float* logits_out, float* emb_out,
                        void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) {
        return enhance_clips_body(c, mix, moff, nclips, ca, caoff, cbw, cboff, den_wav, mixed_wav, logmag_out, phase_out, logits_out, emb_out, s);
    });
}

}  // extern "C"
