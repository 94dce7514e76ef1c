// Context of libnhans_hip.so (C ABI: include/nhans_hip.h): error channel, folded-weight blob, options, activation
// exponents and their calibration, workspace growth, the bracket of an entry point, status and profiling.
#include "host_internal.h"

namespace {

thread_local std::string g_err;

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

constexpr int kActTargetLog2 = 8;

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

__global__ void launch_probe_kernel(int* out) {
    extern __shared__ int probe_lds[];
    probe_lds[threadIdx.x] = threadIdx.x;
    __syncthreads();
    if (out && threadIdx.x == 0) *out = probe_lds[63];
}

}  // namespace

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

static int ws_reserve(nhans_ctx* c, size_t bytes) {
    if (bytes <= c->ws_bytes) return NHANS_OK;
    if (c->ws) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->ws), bytes);
    if (e != hipSuccess) {
        char buf[128];
        snprintf(buf, sizeof buf, "workspace hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return fail(NHANS_ENOMEM, buf);
    }
    c->ws_bytes = bytes;
    return NHANS_OK;
}

int ws_commit(nhans_ctx* c, const WsPlan& p) {
    if (!p.ok()) return fail(NHANS_EINVAL, "workspace plan: more than " + std::to_string(WsPlan::kCap) + " buffers");
    const int rc = ws_reserve(c, p.bytes()); if (rc) return rc;
    p.place(c->ws);         // (only now: the reserve may have freed what the workspace was)
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

Call::Call(nhans_ctx* c_, void* stream) : c(c_), s(static_cast<hipStream_t>(stream)), rc(check_ctx(c_)) {
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
int Call::finish(int body_rc) {
    const int lrc = launch_status();
    if (hipEventRecord(c->tail_ev, s) == hipSuccess) { c->have_tail = true; c->last_stream = s; }
    return body_rc ? body_rc : lrc;
}

// ---- argument checks several units share (slot_check, push_check: the streaming objects) -------------
int slot_check(int S, int slot, const char* fn) {
    if (slot < 0 || slot >= S)
        return fail(NHANS_EINVAL, std::string(fn) + ": slot " + std::to_string(slot) + " outside [0, " + std::to_string(S) + ")");
    return NHANS_OK;
}

// What a push of cnt samples (en: and the end) to stream i may not be, for the three streaming objects and their
// out_counts: `noun` is what the object calls a stream ("stream" / "slot"), `ended` the stream's flag, `uncond` non-null
// where the slot has no conditioning and the call refuses samples for such a slot (it names the calls that set one),
// max_cnt the most samples one push of the object takes.
int push_check(const char* fn, const char* noun, int i, int64_t cnt, bool en, bool ended, const char* uncond, int64_t max_cnt) {
    const std::string who = std::string(fn) + ": " + noun + " " + std::to_string(i);
    if (cnt < 0) return fail(NHANS_EINVAL, who + " has a negative sample count");
    if (ended && (cnt > 0 || en)) return fail(NHANS_EINVAL, who + " has ended");
    if (uncond && (cnt > 0 || en))
        return fail(NHANS_EINVAL, std::string(fn) + ": slot " + std::to_string(i) + " has no conditioning yet (" + uncond + ")");
    if (cnt > max_cnt) return fail(NHANS_EINVAL, std::string(fn) + ": push too large for one call (split it)");
    return NHANS_OK;
}

int offsets_check(const std::string& fn, const char* what, const int64_t* off, int nclips) {
    for (int i = 0; i < nclips; ++i)
        if (off[i + 1] < off[i])
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + ": the " + what + " offsets descend (" +
                                      std::to_string(off[i]) + " -> " + std::to_string(off[i + 1]) + ")");
    return NHANS_OK;
}

int null_clip(const std::string& fn, int i, int64_t n) {
    return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(n) + " samples and a null buffer");
}

int pair_clips(const std::string& fn, const char* verb, const float* est, const int64_t* eoff, const float* tgt, const int64_t* toff,
               int nclips, const void* out, const PairBody& body) {
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (nclips > 0 && (!eoff || !toff || !out))
        return fail(NHANS_EINVAL, fn + ": null offsets or null output with " + std::to_string(nclips) + " clips to " + verb);
    int rc = offsets_check(fn, "estimate", eoff, nclips); if (rc) return rc;
    rc = offsets_check(fn, "target", toff, nclips); if (rc) return rc;
    for (int i = 0; i < nclips; ++i) {
        rc = body(i, est ? est + eoff[i] : nullptr, tgt ? tgt + toff[i] : nullptr, eoff[i + 1] - eoff[i], toff[i + 1] - toff[i]);
        if (rc) return rc;
    }
    return NHANS_OK;
}

// ================================================================================================
extern "C" {

int nhans_abi_version(void) { return NHANS_ABI_VERSION; }
const char* nhans_last_error(void) { return g_err.c_str(); }

int64_t nhans_num_frames(int64_t n) { return n < kWin ? 0 : 1 + (n - kWin) / kHop; }

// The batch of the built-in calibration: two clips -- a two-second mixture of a gliding harmonic voice with syllabic
// amplitude modulation and noise, conditioned once on two noise recordings and once on (silence, noise): an all-zero
// recording is the reference's default `--pos` and drives the tower with the constant silence floor.  Deterministic (LCG).
// mix [2 * n_mix], ca / cb [2 * n_ctx], clip after clip.  calibrate_builtin() and nhans_debug_builtin_batch share it.
constexpr int64_t kBuiltinMix = kWin + (int64_t)kHop * 197, kBuiltinCtx = kWin + (int64_t)kHop * (kCtxFrames - 1);
static void builtin_batch(float* mix, float* ca, float* cb) {
    const int64_t n_mix = kBuiltinMix, n_ctx = kBuiltinCtx;
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
}

// Activation exponents of a fresh context: one pass of the whole path at precision 0 over the built-in batch with every
// tensor's maximum recorded -- a "calibrate" bracket round nhans_enhance_clips of that batch.
static int calibrate_builtin(nhans_ctx* c) {
    const int64_t n_mix = kBuiltinMix, n_ctx = kBuiltinCtx;
    std::vector<float> mix(2 * n_mix), ca(2 * n_ctx), cb(2 * n_ctx);
    builtin_batch(mix.data(), ca.data(), cb.data());
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
    c->tower = tower_geometry(kCtxFrames, kBins);
    c->stack = main_geometry(kMixWin, kBins);
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
    // the blob's directory, for this function alone: every array the launch sequences will dereference is declared in
    // net_weights.h, looked up here once and kept as a pointer in c->net -- or the blob is refused
    std::map<std::string, std::pair<const float*, size_t>> arr;
    const BlobEntry* ent = reinterpret_cast<const BlobEntry*>(static_cast<const char*>(blob) + sizeof(BlobHeader));
    for (uint32_t i = 0; i < h->n_entries; ++i) {
        if (ent[i].offset % 16 || ent[i].offset + ent[i].nfloats * 4 > nbytes) {
            nhans_destroy(c); return fail(NHANS_EINVAL, "blob entry out of range");
        }
        std::string name(ent[i].name, strnlen(ent[i].name, sizeof ent[i].name));
        arr[name] = {reinterpret_cast<const float*>(reinterpret_cast<const char*>(c->blob_dev) + ent[i].offset), ent[i].nfloats};
    }
    // conditioning columns: conv order m0.c1, m0.c2, m1.c1, ...
    int off = 0;
    for (int b = 0; b < 8; ++b) for (int j = 0; j < 2; ++j) { c->cond_off.push_back(off); off += c->stack[b].cout; }
    c->cond_cols = off;
    const std::string bad = resolve_net_weights(c->tower, c->stack, [&](const std::string& name, const float** p, size_t* n) {
        const auto it = arr.find(name);
        if (it == arr.end()) return false;
        *p = it->second.first; *n = it->second.second;
        return true;
    }, &c->net);
    if (!bad.empty()) { nhans_destroy(c); return fail(NHANS_EINVAL, bad); }
    if (act_exp) {
        // (exponents a previous context calibrated for this very blob -- the caller's cache vouches for that: no pass)
        std::copy(act_exp, act_exp + kNumAct, c->act_exp);
        tie_exponents(c);
    } else if (c->net.has_split) {
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
    if (c->drift_tab) (void)hipFree(c->drift_tab);
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
    else if (k == "bss_group_bytes") {
        if (value < 1) return fail(NHANS_EINVAL, "bss_group_bytes < 1");
        c->bss_group_bytes = (size_t)value;
    }
    else if (k == "phase_iters") {
        if (value < 0 || value > kPhaseMaxIters) return fail(NHANS_EINVAL, "phase_iters must be in [0, " + std::to_string(kPhaseMaxIters) + "]");
        c->phase_iters = (int)value;
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
    else if (k == "row_split") {
        if (value < 0 || value > 2) return fail(NHANS_EINVAL, "row_split must be 0, 1 or 2 (2: every conv that can be split, a measurement value)");
        c->row_split = (int)value;
    }
    else if (k == "precision") {
        if (value != 0 && value != 1) return fail(NHANS_EINVAL, "precision must be 0 (f32) or 1 (f16x3)");
        if (value == 1 && !c->net.has_split)
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

int nhans_debug_builtin_batch(float* mix_out, float* ctx_a_out, float* ctx_b_out, int64_t* lengths_out) {
    if (!lengths_out) return fail(NHANS_EINVAL, "built-in batch: null lengths");
    if ((mix_out || ctx_a_out || ctx_b_out) && !(mix_out && ctx_a_out && ctx_b_out))
        return fail(NHANS_EINVAL, "built-in batch: all three arrays or none");
    lengths_out[0] = kBuiltinMix;
    lengths_out[1] = kBuiltinCtx;
    if (mix_out) builtin_batch(mix_out, ctx_a_out, ctx_b_out);
    return NHANS_OK;
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
