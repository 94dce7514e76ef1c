// ---- live PCM sessions (include/nhans_hip.h: nhans_live_*) -----------------------------------------------------------
// One object = an incoming converter (rate_in -> 16 kHz with the fixed peak), an online object and an outgoing converter
// (16 kHz -> rate_out, fed by the wet/dry mix), with the 16 kHz pieces between them in device buffers of the object.  A
// push runs the three stages inside ONE Call on one stream; the stages' own workspace needs (run tables, the online
// staging) follow each other in the context's workspace, which stream order makes safe, and nothing a later stage reads
// lives there.
// An object opened with nhans_interleaved_live_open is the same object whose PCM sides are frames of several channels
// (include/nhans_hip.h: nhans_interleaved_*): only where a slot's samples sit in the caller's buffers differs, which the
// two converters' runs carry (Interleave, host_internal.h) -- the same three stages, launches and snapshots.
// An object that has enabled its full band (include/nhans_hip.h: nhans_fullband_*) also keeps, per slot, the incoming
// samples that have no output yet (FullBand below): one small launch more per push, and the outgoing launch adds the
// input's own band above 8 kHz to what it stores.
#include "host_internal.h"

#include <mutex>

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

// The full band of a live object (nhans_fullband_live_enable; resample.hip: ResidualSource, HighbandSink, hold_kernel):
// per slot a gain and a double-buffered hold of H float32 samples -- the slot's own incoming samples that have no output
// yet, x as the incoming stage's source forms them.  Half cur[i] holds samples [base[i], N) of the stream, N the samples
// the incoming stage has taken; a push that brings samples reads it and writes [E_new, N_new) into the other half, as
// RateStage::hist, so the snapshot of a push is cur and base alone.
struct FullBand {
    bool on = false;
    int64_t H = 0;
    float* hold = nullptr;          // [2][S][H]
    std::vector<float> gain;        // [S]
    struct Slots {
        std::vector<char> cur;
        std::vector<int64_t> base;
    } st;
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
    // nhans_interleaved_live_open: the pushes take frames of Ci channels and return frames of Co, G streams of K slots each
    // -- K = 1 (downmix: the slot is the mean of the frame's channels) or K = Ci = Co (split: slot g K + c is channel c)
    struct Frames {
        bool on = false;
        int Ci = 1, Co = 1, G = 0, K = 1;
    } fr;
    FullBand fb;
    FullBand::Slots undo_fb;
    double* lv_half(int k, int i) const { return lv.state + ((size_t)k * S + i) * kLevelState; }
    float* fb_half(int k, int i) const { return fb.hold + ((size_t)k * S + i) * (size_t)fb.H; }
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
    LevelRun* runs_dev;
    const int rc = ws_upload(c, runs, s, &runs_dev); if (rc) return rc;
    Prof pr(c, s, "live_level");
    launch_level("live_level", runs_dev, (int)runs.size(), s);
    pr.done(9.0 * (double)(ooff[S] - ooff[0]), 8.0 * (double)(ooff[S] - ooff[0]) + (double)runs.size() * 2 * kLevelState * 8);
    return NHANS_OK;
}

// The hold launch of a full-band push: one run per slot whose stream goes on after samples of this push (keep[i] >= 0:
// the first sample its next half holds), reading half cur[i] and the caller's PCM -- slot i's from element pos[i] on --,
// writing the other half.  Host state does not move here: *next is what fb.st becomes once the whole push has gone out.
int live_hold(nhans_live* o, const void* in, const int64_t* pos, const Interleave* il_in, const int64_t* keep, const int64_t* n_old,
              const int64_t* cnt, hipStream_t s, FullBand::Slots* next) {
    nhans_ctx* c = o->c;
    *next = o->fb.st;
    std::vector<HoldRun> runs;
    double samples = 0;
    for (int i = 0; i < o->S; ++i) {
        if (keep[i] < 0) continue;
        const int k = o->fb.st.cur[i];
        runs.push_back({o->fb_half(k, i), o->fb_half(1 - k, i), static_cast<const char*>(in) + pos[i] * rs_elem(o->in_format),
                        (long long)o->fb.st.base[i], (long long)n_old[i], (long long)keep[i], (long long)(n_old[i] + cnt[i]),
                        o->in_format, il_in ? il_in->ch : 0, il_in ? il_in->n : 0});
        next->cur[i] = (char)(1 - k);
        next->base[i] = keep[i];
        samples += (double)(n_old[i] + cnt[i] - keep[i]);
    }
    if (runs.empty()) return NHANS_OK;
    HoldRun* runs_dev;
    const int rc = ws_upload(c, runs, s, &runs_dev); if (rc) return rc;
    Prof pr(c, s, "live_hold");
    launch_hold("live_hold", runs_dev, (int)runs.size(), s);
    pr.done(0, 8.0 * samples);
    return NHANS_OK;
}

// One push, per slot: inoff / outoff are the slots' counts and room -- and, for a mono object, where their pieces are;
// il_in / il_out (an interleaved object; both or neither): where they are in the caller's frames instead.
int live_push_body(nhans_live* o, const char* fn_, const void* in, const int64_t* inoff, const int* end, void* out,
                   const int64_t* outoff, int64_t* counts, hipStream_t s, const Interleave* il_in = nullptr,
                   const Interleave* il_out = nullptr) {
    const std::string fn = fn_;
    if (!inoff || !outoff || !counts) return fail(NHANS_EINVAL, fn + ": null argument");
    nhans_ctx* c = o->c;
    const int S = o->S;
    std::vector<int64_t> moff(S + 1, 0), ooff(S + 1, 0);
    std::vector<int64_t> keep, n_old, cnts, pos;         // (full band only)
    if (o->fb.on) { keep.assign(S, -1); n_old = o->in.st.N; cnts.assign(S, 0); pos.assign(S, 0); }
    int64_t tin = 0, tout = 0;
    for (int i = 0; i < S; ++i) {
        const int64_t cnt = inoff[i + 1] - inoff[i];
        const bool en = end && end[i];
        const int rc = live_check_push(o, fn_, i, cnt, en); if (rc) return rc;
        const LivePlan p = live_plan(o, i, cnt, en);
        if (o->fb.on) {
            cnts[i] = cnt;
            pos[i] = il_in ? il_in->base[i] : inoff[i];
            if (cnt > 0 && !en) {        // (an ended stream emits nothing more: its hold is not read again)
                keep[i] = std::min(p.En, n_old[i] + cnt);
                if (n_old[i] + cnt - keep[i] > o->fb.H) return fail(NHANS_EINVAL, fn + ": internal state bound");
            }
        }
        if (outoff[i + 1] - outoff[i] < p.En - p.Eo)
            return fail(NHANS_EINVAL, fn + ": output room of slot " + std::to_string(i) + " is " +
                                      std::to_string(outoff[i + 1] - outoff[i]) + " samples, " +
                                      std::to_string(p.En - p.Eo) + " needed (nhans_live_out_counts)");
        moff[i + 1] = moff[i] + p.n16;
        ooff[i + 1] = ooff[i] + p.d16;
        tin += cnt; tout += p.En - p.Eo;
    }
    if ((tin > 0 && !in) || (tout > 0 && !out)) return fail(NHANS_EINVAL, fn + ": null buffer");
    int rc = live_reserve(o, (size_t)moff[S], (size_t)ooff[S]); if (rc) return rc;

    // ---- the three stages, the pieces [moff) and [ooff) between them: each commits its host state when its launches
    // went out, and a failure behind it puts it back (an online push undone leaves nothing for nhans_live_rewind) ----
    const RateStage::Streams was_in = o->in.save(), was_out = o->out.save();
    std::vector<int64_t> got(S, 0);
    rc = stage_push(c, o->in, "live_in", {false, o->in_format, 0, 0.f, o->in_denom, false, il_in != nullptr}, in, nullptr, inoff, end,
                    o->mid, moff.data(), got.data(), s, nullptr, il_in);
    if (rc || launch_error_pending()) return rc;          // (a launch error is reported by the entry point; no stage has committed)
    rc = online_push_body(o->on, o->mid, moff.data(), end, o->den, o->mix, ooff.data(), got.data(), s);
    if (rc || launch_error_pending()) { o->in.restore(was_in); return rc; }
    // a failure from here on: both stages that have committed go back
    auto unwind = [&](int status) { o->in.restore(was_in); online_undo(o->on); o->can_rewind = false; return status; };
    // (an object that never enabled its meter takes none of the branches below: launch for launch the push it was)
    std::vector<int64_t> woff;
    LevelMeter::Slots lv_next;
    if (o->lv.on) {
        rc = live_level(o, ooff.data(), end, s, &woff, &lv_next);
        if (rc || launch_error_pending()) return unwind(rc);
    }
    const bool auto_wet = o->lv.on && o->lv.auto_wet;
    const GainTab gains{o->lv.wtab, woff.data()};
    // (nor does an object that never enabled its full band take the ones here)
    FullBand::Slots fb_next;
    std::vector<const float*> halves;
    HighBandIo hb{};
    if (o->fb.on) {
        rc = live_hold(o, in, pos.data(), il_in, keep.data(), n_old.data(), cnts.data(), s, &fb_next);
        if (rc || launch_error_pending()) return unwind(rc);
        for (int i = 0; i < S; ++i) halves.push_back(o->fb_half(o->fb.st.cur[i], i));
        hb = {o->fb.gain.data(), halves.data(), o->fb.st.base.data(), n_old.data(), cnts.data(), pos.data(), in, o->in_format,
              il_in ? il_in->ch : 0, il_in ? il_in->n : 0, o->in_denom};
    }
    rc = stage_push(c, o->out, "live_out",
                    {true, o->out_format, 0, o->wet, o->out_scale, auto_wet, il_out != nullptr, o->fb.on}, o->den,
                    auto_wet || o->wet != 0.f || o->fb.on ? o->mix : nullptr, ooff.data(), end, out, outoff, counts, s,
                    auto_wet ? &gains : nullptr, il_out, o->fb.on ? &hb : nullptr);
    if (rc || launch_error_pending()) return unwind(rc);
    o->undo_in = was_in; o->undo_out = was_out;
    if (o->fb.on) {
        o->undo_fb = o->fb.st;
        o->fb.st = fb_next;
    }
    if (o->lv.on) {
        o->undo_lv = o->lv.st;
        o->lv.st = lv_next;
        o->lv.woff = woff;
    }
    o->can_rewind = true;
    return NHANS_OK;
}

// ---- interleaved frames (include/nhans_hip.h: nhans_interleaved_*) ----
int frames_check_object(const nhans_live* o, const char* fn, bool want_frames, const char* other) {
    if (o->fr.on == want_frames) return NHANS_OK;
    return fail(NHANS_EINVAL, std::string(fn) + (want_frames ? ": the object takes mono pieces per slot (opened with nhans_live_open_slots): "
                                                             : ": the object takes interleaved frames per stream (opened with "
                                                               "nhans_interleaved_live_open): ") + "call " + other);
}

// What a push of cnt[g] frames (end: and the end) to every stream is per slot: the slots' counts as offsets and their end
// flags, after the checks that need no plan -- each slot's own (live_check_push) and, for the K > 1 slots of a split
// stream that the push moves (frames or the end), that they are in step: samples taken, ended flag and look-ahead.
struct FramePush {
    std::vector<int64_t> inoff;     // [S + 1]: slot i brings inoff[i + 1] - inoff[i] frames
    std::vector<int> end;           // [S]
};
int frames_slots(const nhans_live* o, const char* fn_, const int64_t* cnt, const int* end, FramePush* fp) {
    const std::string fn = fn_;
    const int K = o->fr.K;
    fp->inoff.assign(o->S + 1, 0);
    fp->end.assign(o->S, 0);
    for (int g = 0; g < o->fr.G; ++g) {
        const bool en = end && end[g];
        for (int k = 0; k < K; ++k) {
            const int i = g * K + k, i0 = g * K;
            const int rc = live_check_push(o, fn_, i, cnt[g], en); if (rc) return rc;
            if (k > 0 && (cnt[g] > 0 || en)) {
                const char* what = o->in.st.N[i] != o->in.st.N[i0]           ? "samples taken"
                                   : o->in.st.ended[i] != o->in.st.ended[i0] ? "ended flag"
                                   : o->on->la[i] != o->on->la[i0]           ? "look-ahead"
                                   : o->out.st.N[i] != o->out.st.N[i0]       ? "samples the outgoing stage has taken"
                                                                             : nullptr;
                if (what)
                    return fail(NHANS_EINVAL, fn + ": stream " + std::to_string(g) + ": slot " + std::to_string(i) + " differs from slot " +
                                              std::to_string(i0) + " in " + what + " (the channels of a split stream move together: " +
                                              "restart them together, set their look-ahead alike)");
            }
            fp->inoff[i + 1] = fp->inoff[i] + cnt[g];
            fp->end[i] = en;
        }
    }
    return NHANS_OK;
}

// frames stream g emits: those of its first slot, which its other slots share (frames_slots; a last look here)
int frames_plan(const nhans_live* o, const char* fn, const FramePush& fp, int g, int64_t* frames) {
    const int K = o->fr.K;
    for (int k = 0; k < K; ++k) {
        const int i = g * K + k;
        const LivePlan p = live_plan(o, i, fp.inoff[i + 1] - fp.inoff[i], fp.end[i] != 0);
        if (k == 0) *frames = p.En - p.Eo;
        else if (p.En - p.Eo != *frames)
            return fail(NHANS_EINVAL, std::string(fn) + ": stream " + std::to_string(g) + ": slot " + std::to_string(i) +
                                      " differs from slot " + std::to_string(g * K) + " in the frames it would emit");
    }
    return NHANS_OK;
}

int frames_push_body(nhans_live* o, const void* in, const int64_t* inoff, const int* end, void* out, const int64_t* outoff,
                     int64_t* counts, hipStream_t s) {
    const char* fn = "nhans_interleaved_live_push";
    int rc = frames_check_object(o, fn, true, "nhans_live_push"); if (rc) return rc;
    if (!inoff || !outoff || !counts) return fail(NHANS_EINVAL, std::string(fn) + ": null argument");
    const int G = o->fr.G, K = o->fr.K, S = o->S;
    std::vector<int64_t> cnt(G);
    for (int g = 0; g < G; ++g) cnt[g] = inoff[g + 1] - inoff[g];
    FramePush fp;
    rc = frames_slots(o, fn, cnt.data(), end, &fp); if (rc) return rc;
    // per slot: its room is what it needs (the stream's room is checked here, in frames), and where its first sample is
    std::vector<int64_t> room(S + 1, 0), base_in(S), base_out(S), got(S, 0);
    for (int g = 0; g < G; ++g) {
        int64_t frames = 0;
        rc = frames_plan(o, fn, fp, g, &frames); if (rc) return rc;
        if (outoff[g + 1] - outoff[g] < frames)
            return fail(NHANS_EINVAL, std::string(fn) + ": output room of stream " + std::to_string(g) + " is " +
                                      std::to_string(outoff[g + 1] - outoff[g]) + " frames, " + std::to_string(frames) +
                                      " needed (nhans_interleaved_live_out_counts)");
        for (int k = 0; k < K; ++k) {
            const int i = g * K + k;
            room[i + 1] = room[i] + frames;
            base_in[i] = inoff[g] * o->fr.Ci + k;       // (K == 1: the frame's first channel, from which all Ci are summed)
            base_out[i] = outoff[g] * o->fr.Co + k;
        }
    }
    const Interleave il_in{o->fr.Ci, K > 1 ? 1 : o->fr.Ci, base_in.data()}, il_out{o->fr.Co, K > 1 ? 1 : o->fr.Co, base_out.data()};
    rc = live_push_body(o, fn, in, fp.inoff.data(), fp.end.data(), out, room.data(), got.data(), s, &il_in, &il_out);
    if (rc || launch_error_pending()) return rc;
    for (int g = 0; g < G; ++g) counts[g] = got[g * K];
    return NHANS_OK;
}

void live_free(nhans_live* o) {
    if (o->on) nhans_online_close(o->on);
    o->in.release(); o->out.release();
    for (float* p : {o->mid, o->den, o->mix, o->lv.wtab})
        if (p) (void)hipFree(p);
    if (o->lv.state) (void)hipFree(o->lv.state);
    if (o->fb.hold) (void)hipFree(o->fb.hold);
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

namespace {
// the checks and the object of both open functions: `count` slots (mono) or streams of `per` slots each (interleaved)
int live_open_body(const char* fn_, const char* noun, nhans_ctx* c, int count, int per, int rate_in, int in_format, double peak,
                   int rate_out, int out_format, double out_scale, int flags, hipStream_t s, nhans_live** out) {
    const std::string fn = fn_;
    if (count < 1 || count > std::numeric_limits<int>::max() / per) return fail(NHANS_EINVAL, fn + ": " + noun + " must be >= 1");
    for (int fmt : {in_format, out_format})
        if (fmt != kResampleInt16 && fmt != kResampleFloat32)
            return fail(NHANS_EINVAL, fn + ": in_format and out_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32");
    if (!(peak >= 0.0) || !std::isfinite(peak)) return fail(NHANS_EINVAL, fn + ": the peak must be finite and >= 0");
    if (!(out_scale > 0.0) || !std::isfinite(out_scale)) return fail(NHANS_EINVAL, fn + ": out_scale must be finite and > 0");
    if (flags & ~NHANS_LIVE_WET) return fail(NHANS_EINVAL, fn + ": unknown flag");
    const ResampleFilter *fi = nullptr, *fo = nullptr;
    int rc = live_filters(fn_, rate_in, rate_out, &fi, &fo); if (rc) return rc;
    const int nslots = count * per;
    nhans_live* o = new nhans_live();
    o->c = c; o->device = c->device; o->S = nslots; o->in_format = in_format; o->out_format = out_format;
    o->has_wet = (flags & NHANS_LIVE_WET) != 0;
    o->in_denom = peak + 0.000001; o->out_scale = out_scale;
    rc = o->in.alloc(c, fn_, fi, nslots);
    if (!rc) rc = o->out.alloc(c, fn_, fo, nslots);
    if (!rc) rc = online_open_slots_body(c, nslots, o->has_wet, s, &o->on);
    if (rc) { live_free(o); return rc; }
    *out = o;
    return NHANS_OK;
}
}  // namespace

int nhans_live_open_slots(nhans_ctx* c, int nslots, int rate_in, int in_format, double peak, int rate_out, int out_format,
                          double out_scale, int flags, void* stream, nhans_live** out) {
    if (!out) return fail(NHANS_EINVAL, "nhans_live_open_slots: null argument");
    *out = nullptr;
    return ctx_call(c, stream, [&](hipStream_t s) {
        return live_open_body("nhans_live_open_slots", "nslots", c, nslots, 1, rate_in, in_format, peak, rate_out, out_format, out_scale,
                              flags, s, out);
    });
}

int nhans_interleaved_live_open(nhans_ctx* c, int nstreams, int channels_in, int channels_out, int mode, int rate_in, int in_format,
                                double peak, int rate_out, int out_format, double out_scale, int flags, void* stream,
                                nhans_live** out) {
    const std::string fn = "nhans_interleaved_live_open";
    if (!out) return fail(NHANS_EINVAL, fn + ": null argument");
    *out = nullptr;
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        for (int ch : {channels_in, channels_out})
            if (ch < 1 || ch > NHANS_INTERLEAVED_MAX_CHANNELS)
                return fail(NHANS_EINVAL, fn + ": channels_in and channels_out must be in 1 ... " +
                                          std::to_string(NHANS_INTERLEAVED_MAX_CHANNELS) + " (got " + std::to_string(channels_in) +
                                          " and " + std::to_string(channels_out) + ")");
        if (mode != NHANS_INTERLEAVED_DOWNMIX && mode != NHANS_INTERLEAVED_SPLIT)
            return fail(NHANS_EINVAL, fn + ": mode must be NHANS_INTERLEAVED_DOWNMIX or NHANS_INTERLEAVED_SPLIT");
        if (mode == NHANS_INTERLEAVED_SPLIT && channels_in != channels_out)
            return fail(NHANS_EINVAL, fn + ": NHANS_INTERLEAVED_SPLIT needs channels_in == channels_out (got " +
                                      std::to_string(channels_in) + " and " + std::to_string(channels_out) + ")");
        const int K = mode == NHANS_INTERLEAVED_SPLIT ? channels_in : 1;
        const int rc = live_open_body("nhans_interleaved_live_open", "nstreams", c, nstreams, K, rate_in, in_format, peak, rate_out,
                                      out_format, out_scale, flags, s, out);
        if (rc) return rc;
        (*out)->fr.on = true;
        (*out)->fr.Ci = channels_in; (*out)->fr.Co = channels_out; (*out)->fr.G = nstreams; (*out)->fr.K = K;
        return NHANS_OK;
    });
}

int nhans_live_restart(nhans_live* o, int slot) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_restart: null object");
    const int rc = slot_check(o->S, slot, "nhans_live_restart"); if (rc) return rc;
    // (nothing is cleared on the device: streams of 0 samples read none of the carried state, in any of the stages)
    online_restart_slot(o->on, slot);
    o->in.restart(slot); o->out.restart(slot);
    if (o->lv.on) { o->lv.st.h0[slot] = 0; o->lv.woff.clear(); }     // (hop 0 reads none of the carried level state)
    if (o->fb.on) o->fb.st.base[slot] = 0;                           // (a stream of 0 samples has none in its hold)
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_live_set_context(nhans_live* o, int slot, const float* ca, int64_t na, const float* cbw, int64_t nb, void* stream,
                           int64_t* first_frame_out) {
    return object_call(o, "nhans_live_set_context: null object", stream, [&](hipStream_t s) -> int {
        int rc = slot_check(o->S, slot, "nhans_live_set_context"); if (rc) return rc;
        if (!ca || !cbw) return fail(NHANS_EINVAL, "nhans_live_set_context: null argument");
        if (na < 0 || nb < 0) return fail(NHANS_EINVAL, "nhans_live_set_context: negative sample count");
        rc = online_set_context_body(o->on, slot, ca, na, cbw, nb, s, first_frame_out);
        if (!rc && !launch_error_pending()) o->can_rewind = false;
        return rc;
    });
}

int nhans_live_set_embeddings(nhans_live* o, int slot, const float* ea, const float* eb, void* stream, int64_t* first_frame_out) {
    return object_call(o, "nhans_live_set_embeddings: null object", stream, [&](hipStream_t s) -> int {
        int rc = slot_check(o->S, slot, "nhans_live_set_embeddings"); if (rc) return rc;
        if (!ea || !eb) return fail(NHANS_EINVAL, "nhans_live_set_embeddings: null argument");
        rc = online_set_embeddings_body(o->on, slot, ea, eb, s, first_frame_out);
        if (!rc) o->can_rewind = false;
        return rc;
    });
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
    if (o->fr.on) return frames_check_object(o, "nhans_live_out_counts", false, "nhans_interleaved_live_out_counts");
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
    return object_call(o, "nhans_live_push: null object", stream, [&](hipStream_t s) {
        if (o->fr.on) return frames_check_object(o, "nhans_live_push", false, "nhans_interleaved_live_push");
        return live_push_body(o, "nhans_live_push", in, inoff, end, out, outoff, counts, s);
    });
}

int nhans_interleaved_live_out_counts(const nhans_live* o, const int64_t* in_frames, const int* end, int64_t* out_frames) {
    const char* fn = "nhans_interleaved_live_out_counts";
    if (!o || !in_frames || !out_frames) return fail(NHANS_EINVAL, std::string(fn) + ": null argument");
    int rc = frames_check_object(o, fn, true, "nhans_live_out_counts"); if (rc) return rc;
    FramePush fp;
    rc = frames_slots(o, fn, in_frames, end, &fp); if (rc) return rc;
    std::vector<int64_t> frames(o->fr.G, 0);
    for (int g = 0; g < o->fr.G; ++g) {
        rc = frames_plan(o, fn, fp, g, &frames[g]); if (rc) return rc;
    }
    std::copy(frames.begin(), frames.end(), out_frames);
    return NHANS_OK;
}

int nhans_interleaved_live_push(nhans_live* o, const void* in, const int64_t* inoff, const int* end, void* out, const int64_t* outoff,
                                int64_t* counts, void* stream) {
    return object_call(o, "nhans_interleaved_live_push: null object", stream,
                       [&](hipStream_t s) { return frames_push_body(o, in, inoff, end, out, outoff, counts, s); });
}

int nhans_live_rewind(nhans_live* o) {
    if (!o) return fail(NHANS_EINVAL, "nhans_live_rewind: null object");
    if (!o->can_rewind) return fail(NHANS_EINVAL, "nhans_live_rewind: no push to undo (one rewind per push)");
    // (every stage wrote the half of its carried state that it did not read: the halves of before the push are intact)
    o->in.restore(o->undo_in);
    online_undo(o->on);
    o->out.restore(o->undo_out);
    if (o->lv.on) { o->lv.st = o->undo_lv; o->lv.woff.clear(); }
    if (o->fb.on) o->fb.st = o->undo_fb;
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_capture_live_enable(nhans_live* o, void* stream) {
    return object_call(o, "nhans_capture_live_enable: null object", stream,
                       [&](hipStream_t s) { return capture_enable_body(o->on, "nhans_capture_live_enable", s); });
}

int nhans_capture_live_context(nhans_live* o, int n, const int* slots, const int* which, int flags, void* stream,
                               int64_t* first_frame_out) {
    return object_call(o, "nhans_capture_live_context: null object", stream, [&](hipStream_t s) {
        const int rc = capture_context_body(o->on, "nhans_capture_live_context", n, slots, which, flags, s, first_frame_out);
        if (!rc && !launch_error_pending()) o->can_rewind = false;
        return rc;
    });
}

int nhans_capture_live_embeddings(const nhans_live* o, int slot, float* ea, float* eb, void* stream) {
    return object_call(o, "nhans_capture_live_embeddings: null object", stream,
                       [&](hipStream_t s) { return capture_embeddings_body(o->on, "nhans_capture_live_embeddings", slot, ea, eb, s); });
}

// ---- filterbank features (include/nhans_hip.h: nhans_fbank_live_*): the online stage's, slot for slot ----
int nhans_fbank_live_attach(nhans_live* o, nhans_fbank* fb, int flags) {
    if (!o) return fail(NHANS_EINVAL, "nhans_fbank_live_attach: null object");
    return fbank_attach_body(o->on, "nhans_fbank_live_attach", fb, flags);
}

int64_t nhans_fbank_live_read(nhans_live* o, int slot, int plane, float* out, int64_t cap_rows, int64_t* first_frame_out, void* stream) {
    return object_count_call(o, "nhans_fbank_live_read: null object", stream, [&](hipStream_t s) {
        return fbank_read_body(o->on, "nhans_fbank_live_read", slot, plane, out, cap_rows, first_frame_out, s);
    });
}

// ---- level meter and automatic compensation (include/nhans_hip.h: nhans_level_*) ----
int64_t nhans_level_hops(int64_t emitted, int ended) {
    if (emitted < 0) return fail(NHANS_EINVAL, "nhans_level_hops: negative sample count");
    return level_hops(emitted, ended != 0);
}

int nhans_level_live_enable(nhans_live* o, void* stream) {
    return object_call(o, "nhans_level_live_enable: null object", stream, [&](hipStream_t) -> int {
        if (!o->has_wet)
            return fail(NHANS_EINVAL, "nhans_level_live_enable: the object was opened without NHANS_LIVE_WET "
                                      "(the meter reads the mixed round trip)");
        if (o->lv.on) return NHANS_OK;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->lv.state), (size_t)2 * o->S * kLevelState * sizeof(double));
        if (e != hipSuccess)
            return fail(NHANS_ENOMEM, std::string("nhans_level_live_enable: hipMalloc failed: ") + hipGetErrorString(e));
        // (nothing is cleared: a slot's first hop h0 reads none of the state)
        o->lv.st.h0.resize(o->S);
        for (int i = 0; i < o->S; ++i) o->lv.st.h0[i] = level_hops(o->out.st.N[i], o->out.st.ended[i]);
        o->lv.st.cur.assign(o->S, 0);
        o->lv.on = true;
        o->can_rewind = false;
        return NHANS_OK;
    });
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
    return object_call(o, "nhans_level_live_read: null object", stream, [&](hipStream_t s) -> int {
        int rc = slot_check(o->S, slot, "nhans_level_live_read"); if (rc) return rc;
        if (!out) return fail(NHANS_EINVAL, "nhans_level_live_read: null argument");
        if (!o->lv.on) return fail(NHANS_EINVAL, "nhans_level_live_read: the meter is not enabled (nhans_level_live_enable)");
        if (level_hops(o->out.st.N[slot], o->out.st.ended[slot]) <= o->lv.st.h0[slot])
            return fail(NHANS_ESHORT, "nhans_level_live_read: slot " + std::to_string(slot) + " has no final hop yet");
        hipError_t e = hipMemcpyAsync(out, o->lv_half(o->lv.st.cur[slot], slot) + kLevelMeter, 8 * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(NHANS_EHIP, std::string("nhans_level_live_read: ") + hipGetErrorString(e));
        return NHANS_OK;
    });
}

int64_t nhans_level_live_gains(nhans_live* o, int slot, float* out, int64_t cap, void* stream) {
    return object_count_call(o, "nhans_level_live_gains: null object", stream, [&](hipStream_t s) -> int64_t {
        const int rc = slot_check(o->S, slot, "nhans_level_live_gains"); if (rc) return rc;
        if (!o->lv.on) return fail(NHANS_EINVAL, "nhans_level_live_gains: the meter is not enabled (nhans_level_live_enable)");
        const int64_t n = o->lv.woff.empty() ? 0 : o->lv.woff[slot + 1] - o->lv.woff[slot];
        if (!out || n == 0) return n;
        if (cap < n)
            return fail(NHANS_EINVAL, "nhans_level_live_gains: room for " + std::to_string(cap) + " gains, " +
                                      std::to_string(n) + " needed");
        hipError_t e = hipMemcpyAsync(out, o->lv.wtab + o->lv.woff[slot], (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(NHANS_EHIP, std::string("nhans_level_live_gains: ") + hipGetErrorString(e));
        return n;
    });
}

int nhans_level_gains(nhans_ctx* c, const float* den, const float* mix, const int64_t* off, int nclips, int window_hops,
                      double wmax, float* w_out, double* sums_out, void* stream) {
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!off || nclips < 0) return fail(NHANS_EINVAL, "nhans_level_gains: null argument");
        int rc = level_check("nhans_level_gains", window_hops, 0, wmax); if (rc) return rc;
        std::vector<LevelRun> runs;
        int64_t hops = 0;
        for (int i = 0; i < nclips; ++i) {
            const int64_t n = off[i + 1] - off[i];
            if (n < 0) return fail(NHANS_EINVAL, "nhans_level_gains: clip " + std::to_string(i) + " has a negative sample count");
            const int64_t nh = level_hops(n, true);
            if (nh > 0 && (!den || !mix || !w_out)) return fail(NHANS_EINVAL, "nhans_level_gains: null buffer");
            if (nh > 0)
                runs.push_back({den + off[i], mix + off[i], nullptr, nullptr, sums_out ? sums_out + 8 * (size_t)i : nullptr, w_out + hops,
                                (long long)n, 0, (long long)nh, 0, window_hops, wmax});
            hops += nh;
        }
        if (runs.empty()) return NHANS_OK;
        LevelRun* runs_dev;
        rc = ws_upload(c, runs, s, &runs_dev); if (rc) return rc;
        const double n = (double)(off[nclips] - off[0]);
        Prof pr(c, s, "level_gains");
        launch_level("level_gains", runs_dev, (int)runs.size(), s);
        pr.done(9.0 * n, 8.0 * n + 4.0 * (double)hops);
        return NHANS_OK;
    });
}

// ---- full-band output (include/nhans_hip.h: nhans_fullband_*) ----
namespace {
static bool fullband_rate(int r) {
    for (int v : {22050, 24000, 32000, 44100, 48000, 88200, 96000})
        if (v == r) return true;
    return false;
}

// H(r): the most input samples a running stream has without their output.  N - emitted(N) repeats every 20 ms of input
// (r / 50 samples bring 320 at 16 kHz, one pair of hops, and r / 50 outputs) once the first pair has come out, before
// 0.23 s: one second of N covers it for every look-ahead.
static int64_t fullband_hold(int rate) {
    static std::map<int, int64_t> cache;    // (a handful of ints; lives as long as the process)
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    int64_t& H = cache[rate];
    if (H) return H;
    const ResampleFilter *fi = resample_filter(rate, 16000), *fo = resample_filter(16000, rate);
    for (int L = 0; L <= kCenter; ++L)
        for (int64_t n = 0; n <= rate; ++n) {
            const int64_t n16 = resample_emitted(*fi, n, false);
            H = std::max(H, n - resample_emitted(*fo, on_emitted(nhans_num_frames(n16), false, L), false));
        }
    return H;
}
}  // namespace

int64_t nhans_fullband_hold_samples(int rate) {
    if (!fullband_rate(rate))
        return fail(NHANS_EINVAL, "nhans_fullband_hold_samples: " + std::to_string(rate) + " Hz is not a full-band rate (22050, 24000, "
                                  "32000, 44100, 48000, 88200 or 96000 Hz)");
    return fullband_hold(rate);
}

int nhans_fullband_live_enable(nhans_live* o, void* stream) {
    const std::string fn = "nhans_fullband_live_enable";
    return object_call(o, "nhans_fullband_live_enable: null object", stream, [&](hipStream_t) -> int {
        if (o->fb.on) return NHANS_OK;
        const int rate_in = o->in.f->rate_in, rate_out = o->out.f->rate_out;
        if (rate_in != rate_out)
            return fail(NHANS_EINVAL, fn + ": the rates differ (" + std::to_string(rate_in) + " Hz in, " + std::to_string(rate_out) +
                                      " Hz out): the input's high band lines up with an output of its own rate only");
        if (rate_in <= 16000 || !fullband_rate(rate_in))
            return fail(NHANS_EINVAL, fn + ": " + std::to_string(rate_in) + " Hz has no band above the 16 kHz path's (22050 Hz and more)");
        if (!o->has_wet)
            return fail(NHANS_EINVAL, fn + ": the object was opened without NHANS_LIVE_WET (the high band is the input less "
                                      "its mixed round trip)");
        for (int i = 0; i < o->S; ++i)
            if (o->in.st.N[i] != 0 || o->in.st.ended[i] || o->on->st[i].N != 0 || o->out.st.N[i] != 0)
                return fail(NHANS_EINVAL, fn + ": slot " + std::to_string(i) + " has a stream under way (enable after open, or "
                                          "after nhans_live_restart of every slot that has taken samples)");
        const int64_t H = fullband_hold(rate_in);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->fb.hold), (size_t)2 * o->S * (size_t)H * sizeof(float));
        if (e != hipSuccess) return fail(NHANS_ENOMEM, fn + ": hipMalloc failed: " + hipGetErrorString(e));
        // (nothing is cleared: a stream of 0 samples has none in its hold)
        o->fb.H = H;
        o->fb.gain.assign(o->S, 1.f);
        o->fb.st.cur.assign(o->S, 0);
        o->fb.st.base.assign(o->S, 0);
        o->fb.on = true;
        o->can_rewind = false;
        return NHANS_OK;
    });
}

int nhans_fullband_live_set_gain(nhans_live* o, int slot, double gain) {
    const char* fn = "nhans_fullband_live_set_gain";
    if (!o) return fail(NHANS_EINVAL, std::string(fn) + ": null object");
    if (!o->fb.on) return fail(NHANS_EINVAL, std::string(fn) + ": the full band is not enabled (nhans_fullband_live_enable)");
    if (slot != -1) { const int rc = slot_check(o->S, slot, fn); if (rc) return rc; }
    if (!std::isfinite(gain) || gain < 0.0 || gain > 4.0) return fail(NHANS_EINVAL, std::string(fn) + ": the gain must be finite, in [0, 4]");
    for (int i = 0; i < o->S; ++i)
        if (slot == -1 || slot == i) o->fb.gain[i] = (float)gain;
    o->can_rewind = false;
    return NHANS_OK;
}

int nhans_fullband_mix(nhans_ctx* c, const void* x, int x_format, const int64_t* xoff, const float* den, const float* mix,
                       const int64_t* off, int nclips, int rate, double in_denom, double wet, const float* wet_hops, double gain,
                       double out_scale, int out_format, void* out, const int64_t* outoff, void* stream) {
    const std::string fn = "nhans_fullband_mix";
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (!xoff || !off || !outoff || nclips < 0) return fail(NHANS_EINVAL, fn + ": null argument");
        for (int fmt : {x_format, out_format})
            if (fmt != kResampleInt16 && fmt != kResampleFloat32)
                return fail(NHANS_EINVAL, fn + ": x_format and out_format must be NHANS_PCM_INT16 or NHANS_PCM_FLOAT32");
        if (!fullband_rate(rate))
            return fail(NHANS_EINVAL, fn + ": " + std::to_string(rate) + " Hz is not a full-band rate (22050, 24000, 32000, 44100, "
                                      "48000, 88200 or 96000 Hz)");
        if (!(in_denom > 0.0) || !std::isfinite(in_denom)) return fail(NHANS_EINVAL, fn + ": in_denom must be finite and > 0");
        if (!(out_scale > 0.0) || !std::isfinite(out_scale)) return fail(NHANS_EINVAL, fn + ": out_scale must be finite and > 0");
        if (!std::isfinite(wet)) return fail(NHANS_EINVAL, fn + ": the wet factor must be finite");
        if (!std::isfinite(gain) || gain < 0.0 || gain > 4.0) return fail(NHANS_EINVAL, fn + ": the gain must be finite, in [0, 4]");
        const ResampleFilter* f = resample_filter(16000, rate);
        const size_t elem = rs_elem(out_format);
        int64_t t16 = 0, tx = 0, tout = 0;
        for (int i = 0; i < nclips; ++i) {
            const int64_t n16 = off[i + 1] - off[i], nx = xoff[i + 1] - xoff[i];
            if (n16 < 0 || n16 > kMaxResampleClip || nx < 0)
                return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(n16) + " samples at 16 kHz and " +
                                          std::to_string(nx) + " at its own rate (0 ... 2^31 - 1; >= 0)");
            const int64_t no = resample_out_count(*f, n16);
            if (outoff[i + 1] - outoff[i] < no)
                return fail(NHANS_EINVAL, fn + ": output room of clip " + std::to_string(i) + " is " +
                                          std::to_string(outoff[i + 1] - outoff[i]) + " samples, " + std::to_string(no) +
                                          " needed (nhans_resample_out_count)");
            t16 += n16; tx += nx; tout += no;
        }
        if ((t16 > 0 && (!den || !mix)) || (tx > 0 && !x) || (tout > 0 && !out)) return fail(NHANS_EINVAL, fn + ": null buffer");
        std::vector<ResampleRun> runs;
        size_t lds = 0;
        int64_t hops = 0;
        for (int i = 0; i < nclips; ++i) {
            const int64_t n16 = off[i + 1] - off[i];
            const size_t first = runs.size();
            rs_add_runs(runs, &lds, *f, den + off[i], mix + off[i], nullptr, static_cast<char*>(out) + outoff[i] * elem, elem, nullptr, 0,
                        (int)n16, 0, resample_out_count(*f, n16));
            for (size_t k = first; k < runs.size(); ++k) {
                if (wet_hops) { runs[k].wtab = wet_hops + hops; runs[k].hop0 = 0; }
                highband_run(runs[k], (float)gain, nullptr, 0, 0, xoff[i + 1] - xoff[i], static_cast<const char*>(x) + xoff[i] * rs_elem(x_format),
                             x_format, 0, 0, in_denom, (int64_t)(k - first) * kResampleRun);
            }
            hops += level_hops(n16, true);
        }
        if (runs.empty()) return NHANS_OK;
        const float* tab = nullptr;
        const int rc = rs_table(c, f, &tab); if (rc) return rc;
        return rs_launch(c, "fullband_mix", runs, tab, *f, {true, out_format, 0, (float)wet, out_scale, wet_hops != nullptr, false, true}, lds,
                         8.0 * (double)t16, (double)tout * (elem + rs_elem(x_format)), tout, s);
    });
}

void nhans_live_close(nhans_live* o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    (void)hipDeviceSynchronize();
    live_free(o);
}

}  // extern "C"
