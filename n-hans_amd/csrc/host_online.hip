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
#include "host_internal.h"

namespace {

int64_t on_s0(int64_t P) { return std::max<int64_t>(0, P - 2) / kIstftHopsPerBlock * kIstftHopsPerBlock; }
int64_t on_lo(int64_t R, int64_t P) { return std::max<int64_t>(0, std::min<int64_t>(R - kCenter, on_s0(P))); }
// frames that are computed (their L look-ahead rows exist) / frames whose samples are final, for a stream of T frames with
// look-ahead L.  on_lo keeps its form: the window still reaches 17 rows BACK from the next ready frame R = T - L, so
// T - lo = L + (R - lo) <= L + max(17, R - S0) <= 41 rows and R - S0 <= 24 for every L <= 17.
int64_t on_ready(int64_t T, bool ended, int L) { return ended ? T : std::max<int64_t>(0, T - L); }
int64_t on_paired(int64_t T, bool ended, int L) { return ended ? T : on_ready(T, false, L) & ~(int64_t)1; }

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
    WsPlan p;
    float* ctxlm;
    int64_t* tabs[2]; int* blks[2];
    TowerBufs tb;
    p.add(&ctxlm, (size_t)2 * S * kCtxFrames * kBins);
    for (int i = 0; i < 2; ++i) { p.add(&tabs[i], 2 * (S + 1)); p.add(&blks[i], 2 * nb); }
    tower_plan(p, c, &tb);
    int rc = ws_commit(c, p); if (rc) return rc;
    rc = stft_impl(c, ca, caoff, S, kCtxFrames, ctxlm, nullptr, tabs[0], blks[0], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, cbw, cboff, S, kCtxFrames, ctxlm + (size_t)S * kCtxFrames * kBins, nullptr, tabs[1], blks[1], nullptr, s);
    if (rc) return rc;
    nhans_online* o = nullptr;
    rc = online_alloc(c, S, want_mixed, true, "nhans_online_open", &o); if (rc) return rc;
    rc = embed_impl(c, ctxlm, 2 * S, o->emb, tb, s);
    if (rc) { (void)hipFree(o->emb); (void)hipFree(o->state); delete o; return rc; }
    *out = o;
    return NHANS_OK;
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

}  // namespace

int64_t on_emitted(int64_t T, bool ended, int L) {
    if (!ended) return (int64_t)kHop * on_paired(T, false, L);
    return T == 0 ? 0 : (T - 1) * kHop + kWin;
}

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
    o->fb.forget();
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
    if (o->fb.on) o->fb.cnt[slot] = 0;
    o->can_rewind = false;
}

int online_set_context_body(nhans_online* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb_,
                            hipStream_t s, int64_t* first_frame) {
    nhans_ctx* c = o->c;
    int rc = slot_check(o->S, slot, "nhans_online_set_context"); if (rc) return rc;
    if (!ca || !cbw) return fail(NHANS_EINVAL, "nhans_online_set_context: null argument");
    if (na < 0 || nb_ < 0) return fail(NHANS_EINVAL, "nhans_online_set_context: negative sample count");
    const int64_t aoff[2] = {0, na}, boff[2] = {0, nb_};
    const size_t nb = std::max(stft_blocks(aoff, 1, kCtxFrames), stft_blocks(boff, 1, kCtxFrames));
    WsPlan p;
    float *ctxlm, *rows;
    int64_t* tabs[2]; int* blks[2];
    TowerBufs tb;
    p.add(&ctxlm, (size_t)2 * kCtxFrames * kBins);
    p.add(&rows, 2 * kEmb);
    for (int i = 0; i < 2; ++i) { p.add(&tabs[i], 4); p.add(&blks[i], 2 * nb); }
    tower_plan(p, c, &tb);
    rc = ws_commit(c, p); if (rc) return rc;
    rc = stft_impl(c, ca, aoff, 1, kCtxFrames, ctxlm, nullptr, tabs[0], blks[0], nullptr, s); if (rc) return rc;
    rc = stft_impl(c, cbw, boff, 1, kCtxFrames, ctxlm + (size_t)kCtxFrames * kBins, nullptr, tabs[1], blks[1], nullptr, s);
    if (rc) return rc;
    // (the tower writes workspace rows, not the object's: a failure leaves the slot's conditioning as it was)
    rc = embed_impl(c, ctxlm, 2, rows, tb, s); if (rc) return rc;
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
//   online_fbank    (a filterbank attached: nhans_fbank_online_attach) the push's denoised and centre rows -> feature rows
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
    const bool feats = o->fb.on && F > 0;
    WsPlan ws;
    float *wav, *nlm, *nph, *win, *ctr, *dnew, *yden, *yph, *ylm, *tden, *tmix = nullptr;
    int64_t *tab_st, *tab_is; int *blk_st, *blk_is, *rb;
    OnlineCopy* runs_dev; StackBufs sb{}; FbankRun* fb_runs = nullptr;
    ws.add(&wav, soff[S]);
    ws.add(&nlm, NF * kBins);
    ws.add(&nph, NF * kBins);
    ws.add(&win, WR * kBins);
    ws.add(&ctr, F * kBins);
    ws.add(&dnew, F * kBins);
    ws.add(&yden, Y * kBins);
    ws.add(&yph, Y * kBins);
    ws.add(&ylm, Y * kBins);
    ws.add(&tden, ooff[S]);
    if (o->mixed) ws.add(&tmix, ooff[S]);
    ws.add(&tab_st, 2 * (S + 1));
    ws.add(&tab_is, 2 * (S + 1));
    ws.add(&blk_st, 2 * nb_st);
    ws.add(&blk_is, 2 * nb_is);
    ws.add(&rb, F);
    ws.add(&runs_dev, nrun_cap);
    if (F > 0) stack_plan(ws, c, F, S, wf, &sb);
    if (feats) ws.add(&fb_runs, 2);
    int rc = ws_commit(c, ws); if (rc) return rc;
    if (feats) {
        // (before anything goes out: a failed allocation leaves the object and the rows of the last push as they were)
        const size_t need = (size_t)(o->fb.mixed ? 2 : 1) * F * o->fb.t.n_out;
        if (need > o->fb.cap) {
            const size_t want = std::max<size_t>({need, 2 * o->fb.cap, 4096});
            float* q = nullptr;
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&q), want * 4);
            if (e != hipSuccess) return fail(NHANS_ENOMEM, std::string("nhans_online_push: hipMalloc failed: ") + hipGetErrorString(e));
            if (o->fb.rows) (void)hipFree(o->fb.rows);      // (hipFree waits for the device: no earlier read still copies from it)
            o->fb.rows = q; o->fb.cap = want;
            o->fb.forget();
        }
    }
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
    o->fb.forget();      // (from here on the feature rows of the last push may be overwritten; set again below, with the host state)
    rc = h2d(c, runs_dev, runs, s); if (rc) return rc;
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
        rc = h2d(c, sb.f_clip, h_clip, s); if (rc) return rc;
        rc = h2d(c, sb.f_t, h_t, s); if (rc) return rc;
        rc = h2d(c, sb.f_T, h_T, s); if (rc) return rc;
        rc = h2d(c, rb, h_rb, s); if (rc) return rc;
        rc = mask_net_run(c, win, rb, ctr, F, S, o->emb, o->emb + (size_t)S * kEmb, nullptr, dnew, sb, wf, s);
        if (rc) return rc;
        if (launch_error_pending()) return NHANS_OK;      // (reported by the entry point; nothing below runs on it)
        if (feats) {
            // (the push's rows are compact, stream after stream, in dnew and in ctr: one run per plane whatever S is)
            const FbankRows planes[2] = {{dnew, o->fb.rows, F}, {ctr, o->fb.rows + (size_t)F * o->fb.t.n_out, F}};
            rc = fbank_launch(c, o->fb.t, "online_fbank", planes, o->fb.mixed ? 2 : 1, fb_runs, s); if (rc) return rc;
        }
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
    if (o->fb.on) {
        o->fb.F = F;
        for (int i = 0; i < S; ++i) { o->fb.off[i] = foff[i]; o->fb.cnt[i] = foff[i + 1] - foff[i]; o->fb.first[i] = pl[i].Ro; }
    }
    return NHANS_OK;
}

// ---- filterbank features of a stream (include/nhans_hip.h: nhans_fbank_online_*) ------------------------------------------
int fbank_attach_body(nhans_online* o, const char* fn_, const nhans_fbank* fb, int flags) {
    const std::string fn = fn_;
    if (flags & ~NHANS_FBANK_MIXED) return fail(NHANS_EINVAL, fn + ": unknown flag");
    if (!fb && flags) return fail(NHANS_EINVAL, fn + ": flags must be 0 when detaching");
    if (fb && fb->device != o->device) return fail(NHANS_EINVAL, fn + ": the filterbank lives on another device than the object");
    const hipError_t e = hipSetDevice(o->device);
    if (e != hipSuccess) return fail(NHANS_EHIP, fn + ": hipSetDevice: " + hipGetErrorString(e));
    FbankTable t;
    if (fb) { const int rc = fbank_table_clone(fb->t, fn_, &t); if (rc) return rc; }
    fbank_table_free(&o->fb.t);
    o->fb.t = t;
    o->fb.on = fb != nullptr;
    o->fb.mixed = (flags & NHANS_FBANK_MIXED) != 0;
    o->fb.F = 0;
    o->fb.off.assign(o->S, 0); o->fb.cnt.assign(o->S, 0); o->fb.first.assign(o->S, 0);
    return NHANS_OK;
}

int64_t fbank_read_body(nhans_online* o, const char* fn_, int slot, int plane, float* out, int64_t cap_rows, int64_t* first_frame,
                        hipStream_t s) {
    const std::string fn = fn_;
    if (!o->fb.on) return fail(NHANS_EINVAL, fn + ": no filterbank is attached (nhans_fbank_online_attach / nhans_fbank_live_attach)");
    const int rc = slot_check(o->S, slot, fn_); if (rc) return rc;
    if (plane != 0 && !(plane == 1 && o->fb.mixed))
        return fail(NHANS_EINVAL, fn + ": plane " + std::to_string(plane) + (plane == 1 ? " needs an attach with NHANS_FBANK_MIXED"
                                                                                        : " outside 0 (denoised) and 1 (mixed)"));
    const int64_t n = o->fb.cnt[slot];
    if (first_frame) *first_frame = n > 0 ? o->fb.first[slot] : on_ready(o->st[slot].T, o->st[slot].ended, o->la[slot]);
    if (!out || n == 0) return n;
    if (cap_rows < n) return fail(NHANS_EINVAL, fn + ": room for " + std::to_string(cap_rows) + " rows, " + std::to_string(n) + " needed");
    const float* src = o->fb.rows + ((size_t)plane * o->fb.F + o->fb.off[slot]) * o->fb.t.n_out;
    HIP_TRY(hipMemcpyAsync(out, src, (size_t)n * o->fb.t.n_out * 4, hipMemcpyDeviceToDevice, s));
    return n;
}

// ---- conditioning captured from a slot's own stream (include/nhans_hip.h: nhans_capture_*) --------------------------------
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
    WsPlan p;
    float *clips, *ctxlm, *rows;
    int64_t* tabs; int* blks;
    CaptureEntry* ent_dev;
    TowerBufs tb;
    p.add(&clips, (size_t)n * kCaptureSamples);
    p.add(&ctxlm, (size_t)n * kCtxFrames * kBins);
    p.add(&rows, (size_t)n * kEmb);
    p.add(&tabs, 2 * (n + 1));
    p.add(&blks, 2 * nb);
    p.add(&ent_dev, n);
    tower_plan(p, c, &tb);
    int rc = ws_commit(c, p); if (rc) return rc;
    std::vector<CaptureEntry> ent(n);
    for (int k = 0; k < n; ++k)
        ent[k] = {o->ring + (size_t)slots[k] * kCaptureSamples, clips + (size_t)k * kCaptureSamples,
                  (int)(o->st[slots[k]].N % kCaptureSamples), flags & NHANS_CAPTURE_NORMALISE};
    rc = h2d(c, ent_dev, ent, s); if (rc) return rc;
    {
        Prof pr(c, s, "capture_clip_kernel");
        launch_capture_clip(ent_dev, n, s);
        pr.done(0, ((flags & NHANS_CAPTURE_NORMALISE) ? 12.0 : 8.0) * n * kCaptureSamples);
    }
    rc = stft_impl(c, clips, soff.data(), n, kCtxFrames, ctxlm, nullptr, tabs, blks, nullptr, s); if (rc) return rc;
    // (the tower writes workspace rows, not the object's: a failure leaves every slot's conditioning as it was)
    rc = embed_impl(c, ctxlm, n, rows, tb, s); if (rc) return rc;
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

// ================================================================================================
extern "C" {

int nhans_online_open(nhans_ctx* c, int nstreams, const float* ca, const int64_t* caoff, const float* cbw,
                      const int64_t* cboff, int want_mixed, void* stream, nhans_online** out) {
    return ctx_call(c, stream, [&](hipStream_t s) { return online_open_body(c, nstreams, ca, caoff, cbw, cboff, want_mixed, s, out); });
}

int nhans_online_open_slots(nhans_ctx* c, int nslots, int want_mixed, void* stream, nhans_online** out) {
    return ctx_call(c, stream, [&](hipStream_t s) { return online_open_slots_body(c, nslots, want_mixed, s, out); });
}

int nhans_online_restart(nhans_online* o, int slot) {
    if (!o) return fail(NHANS_EINVAL, "nhans_online_restart: null object");
    const int rc = slot_check(o->S, slot, "nhans_online_restart"); if (rc) return rc;
    online_restart_slot(o, slot);
    return NHANS_OK;
}

int nhans_online_set_context(nhans_online* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb,
                             void* stream, int64_t* first_frame_out) {
    return object_call(o, "nhans_online_set_context: null object", stream,
                       [&](hipStream_t s) { return online_set_context_body(o, slot, ca, na, cbw, nb, s, first_frame_out); });
}

int nhans_online_set_embeddings(nhans_online* o, int slot, const float* ea, const float* eb, void* stream,
                                int64_t* first_frame_out) {
    return object_call(o, "nhans_online_set_embeddings: null object", stream,
                       [&](hipStream_t s) { return online_set_embeddings_body(o, slot, ea, eb, s, first_frame_out); });
}

int nhans_online_push(nhans_online* o, const float* in, const int64_t* inoff, const int* end, float* den_out,
                      float* mix_out, const int64_t* outoff, int64_t* counts, void* stream) {
    return object_call(o, "null object", stream,
                       [&](hipStream_t s) { return online_push_body(o, in, inoff, end, den_out, mix_out, outoff, counts, s); });
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
    fbank_table_free(&o->fb.t);
    if (o->fb.rows) (void)hipFree(o->fb.rows);
    delete o;
}

int nhans_fbank_online_attach(nhans_online* o, nhans_fbank* fb, int flags) {
    if (!o) return fail(NHANS_EINVAL, "nhans_fbank_online_attach: null object");
    return fbank_attach_body(o, "nhans_fbank_online_attach", fb, flags);
}

int64_t nhans_fbank_online_read(nhans_online* o, int slot, int plane, float* out, int64_t cap_rows, int64_t* first_frame_out,
                                void* stream) {
    return object_count_call(o, "nhans_fbank_online_read: null object", stream, [&](hipStream_t s) {
        return fbank_read_body(o, "nhans_fbank_online_read", slot, plane, out, cap_rows, first_frame_out, s);
    });
}

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
    return object_call(o, "nhans_capture_enable: null object", stream,
                       [&](hipStream_t s) { return capture_enable_body(o, "nhans_capture_enable", s); });
}

int nhans_capture_context(nhans_online* o, int n, const int* slots, const int* which, int flags, void* stream,
                          int64_t* first_frame_out) {
    return object_call(o, "nhans_capture_context: null object", stream,
                       [&](hipStream_t s) { return capture_context_body(o, "nhans_capture_context", n, slots, which, flags, s, first_frame_out); });
}

int nhans_capture_embeddings(const nhans_online* o, int slot, float* ea, float* eb, void* stream) {
    return object_call(o, "nhans_capture_embeddings: null object", stream,
                       [&](hipStream_t s) { return capture_embeddings_body(o, "nhans_capture_embeddings", slot, ea, eb, s); });
}

}  // extern "C"
