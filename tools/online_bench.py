"""Online enhancement (nhans_online_*): push wall time and real-time factor for S live streams per object and pushes of
H hops (H x 10 ms of audio per stream), f16x3, synthetic weights.  One JSON line per (S, H):
  push_ms_p50 / p99   host clock around push + device synchronise, after a warm-up of every shape
  kernel_ms_per_push  sum of the per-kernel hipEvent times of nhans_profile_json over a separate profiled pass
  realtime_factor     S x pushed audio seconds / p50 push time (streams one GPU keeps up with per ... of real time)
  latency_ms          the algorithmic latency range from the output contract (look-ahead + one window, +- one hop)
    python tools/online_bench.py [--streams 1,8,64,256] [--hops 1,4,16] [--pushes 60] [--in_rate 48000] [--out_rate 48000]
                                 [--lookahead L]
  (--lookahead L, 0 ... 17: every stream at look-ahead L -- the line carries "lookahead" and the latency_ms of that L; the
   default 17 makes no look-ahead call at all, so it also runs on a library from before the option: $NHANS_LIB)
  (--in_rate / --out_rate: the pieces are int16 at in_rate and come back at out_rate, each through a device rate
   converter of its own -- nhans_amd/resample.py; the line then carries "in_rate" / "out_rate" and the longer latency)
  (--live, with both rates: the same pushes through a live.LiveSession -- nhans_live_push, one C call per push, the
   16 kHz pieces handed over on the device, int16 in and int16 out -- instead of OnlineEnhancer; the line carries
   "mode": "live".  --out F appends the lines to F)

--churn: a long-lived object whose callers come and go (nhans_online_open_slots).  Per (slots S, active k) it prints
three lines, each with push p50 / p99 over the same pushes of H hops per active stream:
  mode "fixed"   a k-stream nhans_online_open object (what k callers cost when nobody joins or leaves; this mode also
                 runs on a library from before the slot functions: $NHANS_LIB, for a same-box A/B)
  mode "slots"   S slots, k of them active, nobody joins or leaves (idle slots should be free)
                 (both with kernel_ms_per_push, cond_proj_ms_per_push and launches_per_push from a profiled pass)
  mode "churn"   the same, and every J-th push one stream leaves with `end` and one joins an idle slot (restart + by
                 turns set_context and set_embeddings); the wall time of the two set calls, each followed by a device
                 synchronise, is reported on its own (p50 over the joins; set_embeddings gets rows computed beforehand)
    python tools/online_bench.py --churn [--slots 64,256] [--active 16] [--every 8] [--hops 1] [--pushes 240] [--out F]

--capture: what the sample history (nhans_capture_enable) costs a push and what a capture costs.  Per (S, H) one line
with mode "capture": push p50 / p99 of an S-slot object with the history disabled and of its twin with it enabled, the
same pushes by turns (launches_per_push of both from a profiled pass), and the wall time, device synchronise included,
of a one-entry capture_context beside a set_context of the same slot (p50 / max over --captures calls of each).  On a
library from before the capture functions ($NHANS_LIB, for a same-box A/B) the enabled and capture figures are null and
the line still carries the disabled push and set_context.
    python tools/online_bench.py --capture [--streams 1,8] [--hops 1,4] [--pushes 200] [--captures 20] [--out F]

--levels: what the level meter and the automatic wet factor (nhans_level_*) cost a live push.  Per (S, H) one line with
mode "levels": push p50 / p99 of three S-slot live.LiveSession objects opened with the mixed round trip (48 kHz int16 in
and out unless --in_rate / --out_rate say otherwise), the same pushes by turns -- "never" (no level call at all),
"enabled" (enable_levels(), fixed factor 0.25) and "auto" (set_auto_wet(200, 1.0)) --, and launches_per_push and the
live_level kernel time of each from a profiled pass.  On a library from before the level functions ($NHANS_LIB, for a
same-box A/B) only "never" is there and the other figures are null.
    python tools/online_bench.py --levels [--streams 1,16,64] [--hops 2] [--pushes 200] [--out F]

--fullband: what the full band (nhans_fullband_*) costs a live push.  Per (S, H) one line with mode "fullband": push p50 /
p99 of two S-slot live.LiveSession objects opened with the mixed round trip (48 kHz int16 in and out unless --in_rate
says otherwise), the same pushes by turns -- "never" (no full-band call at all) and "enabled" (enable_fullband(), gain
1) --, and launches_per_push and the live_in / live_out / live_hold kernel times of each from a profiled pass.  On a
library from before the functions ($NHANS_LIB, for a same-box A/B) only "never" is there.
    python tools/online_bench.py --fullband [--streams 1,16] [--hops 1,2] [--pushes 200] [--lookahead 2] [--out F]

--interleaved: what interleaved frames (nhans_interleaved_*) cost a live push.  Per (S, H) one line with mode
"interleaved": push p50 / p99 of three live.LiveSession objects of S SLOTS each, 48 kHz int16 in and out unless --in_rate /
--out_rate say otherwise, the same pushes by turns -- "mono" (S mono slots), "downmix" (S stereo streams, one slot each,
stereo out) and "split" (S / 2 stereo streams, two slots each; S even) --, and launches_per_push and the live_in / live_out
kernel times of each from a profiled pass.  On a library from before the functions ($NHANS_LIB, for a same-box A/B) only
"mono" is there and the other figures are null.
    python tools/online_bench.py --interleaved [--streams 2,16,64] [--hops 2] [--pushes 200] [--out F]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nhans_amd  # noqa: E402,F401
from nhans_amd import apply, engine, hip, live, online, spec, synth  # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def churn(a):
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    audio = apply.normalise(synth.mixture(1, 30.0))
    H = int(a.hops.split(",")[0])
    n = H * spec.HOP
    k = a.active
    empty = np.zeros(0, np.float32)
    has_slots = hasattr(hip.load(), "nhans_online_open_slots")
    rows = None
    if has_slots:
        wav = torch.from_numpy(np.concatenate([ca, cb])).to(eng.device)
        lm, _ = eng.stft_features(wav, [0, len(ca), len(ca) + len(cb)], max_frames=spec.NOISE_WIN, want_phase=False)
        rows = eng.embed(lm.reshape(2, spec.NOISE_WIN, spec.BINS))
    out = open(a.out, "a") if a.out else None

    def report(mode, S, ts, extra):
        p50, p99 = float(np.percentile(ts, 50)), float(np.percentile(ts, 99))
        line = {"mode": mode, "slots": S, "active": k, "hops_per_push": H, "push_audio_ms": H * 10,
                "push_ms_p50": round(p50, 3), "push_ms_p99": round(p99, 3), "pushes": len(ts),
                "realtime_factor": round(k * H * 0.010 / (p50 / 1e3), 2)}
        line.update(extra)
        line.update({"lib": os.path.basename(os.environ.get("NHANS_LIB") or "tree"), "precision": "f16x3",
                     "weights": "synthetic seed 7"})
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    for S in [int(s) for s in a.slots.split(",")]:
        for mode in ("fixed", "slots", "churn"):
            if mode != "fixed" and not has_slots:
                continue
            if mode == "fixed":
                enh = online.OnlineEnhancer(eng, [ca] * k, [cb] * k)
                active, idle = list(range(k)), []
            else:
                enh = online.OnlineEnhancer.open_slots(eng, S)
                active, idle = list(range(k)), list(range(k, S))
                for i in active:
                    enh.set_context(i, ca, cb)
            pos = [0]

            def push(leaver=None):
                i = pos[0] % (len(audio) - n)
                pos[0] += n
                chunks, end = [empty] * enh.S, [False] * enh.S
                for j in active:
                    chunks[j] = audio[i:i + n]
                if leaver is not None:
                    end[leaver] = True
                enh.push(chunks, end)

            for _ in range(40):
                push()
            torch.cuda.synchronize()
            ts, t_ctx, t_emb = [], [], []
            for it in range(a.pushes):
                leaver = active[0] if mode == "churn" and it % a.every == a.every - 1 else None
                ts.append(_timed(lambda: push(leaver)))
                if leaver is not None:
                    active.pop(0)
                    idle.append(leaver)
                    j = idle.pop(0)
                    enh.restart(j)
                    if len(t_ctx) <= len(t_emb):
                        t_ctx.append(_timed(lambda: enh.set_context(j, ca, cb)))
                    else:
                        t_emb.append(_timed(lambda: enh.set_embeddings(j, rows[0], rows[1])))
                    active.append(j)
            extra = {}
            if mode != "churn":
                # where a difference between "fixed" and "slots" comes from: device time (and cond_proj's share of it,
                # the one kernel whose grid follows the slot count) against the host side of a push
                eng.set_option("profile", 1)
                eng.profile_reset()
                for _ in range(10):
                    push()
                prof = eng.profile()
                eng.set_option("profile", 0)
                extra = {"kernel_ms_per_push": round(sum(v["ms"] for v in prof.values()) / 10, 3),
                         "cond_proj_ms_per_push": round(prof.get("cond_proj", {"ms": 0.0})["ms"] / 10, 4),
                         "launches_per_push": sum(v["calls"] for v in prof.values()) / 10}
            enh.close()
            if mode == "churn":
                extra = {"churn_every": a.every, "joins": len(t_ctx) + len(t_emb),
                         "set_context_ms_p50": round(float(np.percentile(t_ctx, 50)), 3) if t_ctx else None,
                         "set_context_ms_max": round(float(np.max(t_ctx)), 3) if t_ctx else None,
                         "set_embeddings_ms_p50": round(float(np.percentile(t_emb, 50)), 3) if t_emb else None,
                         "set_embeddings_ms_max": round(float(np.max(t_emb)), 3) if t_emb else None}
            report(mode, S, ts, extra)
    eng.close()
    return 0


def capture(a):
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    audio = apply.normalise(synth.mixture(1, 30.0))
    has = hasattr(hip.load(), "nhans_capture_context")
    out = open(a.out, "a") if a.out else None
    pct = lambda v, q: round(float(np.percentile(v, q)), 3) if len(v) else None
    for S in [int(s) for s in a.streams.split(",")]:
        for H in [int(h) for h in a.hops.split(",")]:
            n = H * spec.HOP
            objs = {"disabled": online.OnlineEnhancer(eng, [ca] * S, [cb] * S)}
            if has:
                objs["enabled"] = online.OnlineEnhancer(eng, [ca] * S, [cb] * S)
                objs["enabled"].enable_capture()
            pos = {k: 0 for k in objs}

            def push(k):
                i = pos[k] % (len(audio) - n)
                pos[k] += n
                objs[k].push([audio[i:i + n]] * S)

            # (past the look-ahead, and past the 32,240 samples a capture needs)
            for k in objs:
                objs[k].push([audio[:online.CAPTURE_SAMPLES]] * S)
                pos[k] = online.CAPTURE_SAMPLES
                for _ in range(40):
                    push(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in objs}
            for _ in range(a.pushes):
                for k in objs:
                    ts[k].append(_timed(lambda: push(k)))
            launches = {}
            for k in objs:
                eng.set_option("profile", 1)
                eng.profile_reset()
                for _ in range(10):
                    push(k)
                launches[k] = sum(v["calls"] for v in eng.profile().values()) / 10
                eng.set_option("profile", 0)
            t_set, t_cap = [], []
            for _ in range(a.captures):
                t_set.append(_timed(lambda: objs["disabled"].set_context(0, ca, cb)))
                if has:
                    t_cap.append(_timed(lambda: objs["enabled"].capture_context(0, "b")))
            for o in objs.values():
                o.close()
            line = {"mode": "capture", "streams": S, "hops_per_push": H, "push_audio_ms": H * 10, "pushes": a.pushes}
            for k in ("disabled", "enabled"):
                line["push_ms_p50_" + k] = pct(ts.get(k, []), 50)
                line["push_ms_p99_" + k] = pct(ts.get(k, []), 99)
                line["launches_per_push_" + k] = launches.get(k)
            line.update({"set_context_ms_p50": pct(t_set, 50), "set_context_ms_max": pct(t_set, 100),
                         "capture_context_ms_p50": pct(t_cap, 50), "capture_context_ms_max": pct(t_cap, 100),
                         "captures": a.captures, "lib": os.path.basename(os.environ.get("NHANS_LIB") or "tree"),
                         "precision": "f16x3", "weights": "synthetic seed 7"})
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
    eng.close()
    return 0


def fbank_cost(a):
    """--fbank: push p50 / p99 of an S-stream object with nothing attached and of its twin with an 80-band HTK filterbank
    attached (one online_fbank launch more per push that computes frames, and one features() read of slot 0), the two
    alternating push by push; then the offline kernel alone: nhans_fbank_rows over 256 x 998 rows, --pushes calls, as bytes
    moved (804 read + 4 n_mels written per row) per second -- by the library's own events around the launch (option
    "profile": the kernel), and by events around the whole Python call (which also wait for the host to get there)."""
    from nhans_amd import fbank
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    audio = apply.normalise(synth.mixture(1, 30.0))
    fb = fbank.Filterbank(80)
    out = open(a.out, "a") if a.out else None
    pct = lambda v, q: round(float(np.percentile(v, q)), 3) if len(v) else None

    def emit(line):
        line.update({"lib": os.path.basename(os.environ.get("NHANS_LIB") or "tree"), "precision": "f16x3",
                     "weights": "synthetic seed 7"})
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    for S in [int(s) for s in a.streams.split(",")]:
        for H in [int(h) for h in a.hops.split(",")]:
            n = H * spec.HOP
            objs = {"detached": online.OnlineEnhancer(eng, [ca] * S, [cb] * S),
                    "attached": online.OnlineEnhancer(eng, [ca] * S, [cb] * S),
                    "attached_read": online.OnlineEnhancer(eng, [ca] * S, [cb] * S)}
            objs["attached"].enable_fbank(fb)
            objs["attached_read"].enable_fbank(fb)
            pos = {k: 0 for k in objs}

            def push(k):
                i = pos[k] % (len(audio) - n)
                pos[k] += n
                objs[k].push([audio[i:i + n]] * S)
                if k == "attached_read":
                    objs[k].features(0)

            for k in objs:
                for _ in range(40):
                    push(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in objs}
            for _ in range(a.pushes):
                for k in objs:
                    ts[k].append(_timed(lambda: push(k)))
            launches = {}
            for k in objs:
                eng.set_option("profile", 1)
                eng.profile_reset()
                for _ in range(10):
                    push(k)
                launches[k] = sum(v["calls"] for v in eng.profile().values()) / 10
                eng.set_option("profile", 0)
            for o in objs.values():
                o.close()
            line = {"mode": "fbank", "streams": S, "hops_per_push": H, "push_audio_ms": H * 10, "pushes": a.pushes, "n_mels": 80}
            for k in objs:
                line["push_ms_p50_" + k] = pct(ts[k], 50)
                line["push_ms_p99_" + k] = pct(ts[k], 99)
                line["launches_per_push_" + k] = launches[k]
            emit(line)
    rows = torch.empty((256 * 998, spec.BINS), dtype=torch.float32, device=eng.device).uniform_(-31.5, 16.0)
    for _ in range(5):
        eng.fbank_rows(rows, fb)
    ms = []
    for _ in range(a.pushes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.fbank_rows(rows, fb)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    nbytes = rows.shape[0] * 4.0 * (spec.BINS + fb.n_mels)
    eng.set_option("profile", 1)
    eng.profile_reset()
    for _ in range(a.pushes):
        eng.fbank_rows(rows, fb)
    prof = eng.profile()["fbank_rows"]
    eng.set_option("profile", 0)
    kernel_ms = prof["ms"] / prof["calls"]
    emit({"mode": "fbank_rows", "rows": rows.shape[0], "n_mels": fb.n_mels, "bytes": nbytes, "calls": len(ms),
          "kernel_ms_mean": round(kernel_ms, 4), "kernel_gbytes_per_s": round(nbytes / (kernel_ms * 1e-3) / 1e9, 1),
          "call_ms_p50": pct(ms, 50), "call_ms_min": round(min(ms), 4),
          "call_gbytes_per_s_p50": round(nbytes / (pct(ms, 50) * 1e-3) / 1e9, 1)})
    fb.close()
    eng.close()
    return 0


def levels(a):
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    rate_in, rate_out = a.in_rate or 48000, a.out_rate or 48000
    idx = (np.arange(int(30.0 * rate_in)) * float(spec.FS) / rate_in).astype(np.int64)
    audio = synth.mixture(1, 30.0)[np.minimum(idx, int(30.0 * spec.FS) - 1)]
    has = hasattr(hip.load(), "nhans_level_hops")
    out = open(a.out, "a") if a.out else None
    pct = lambda v, q: round(float(np.percentile(v, q)), 3) if len(v) else None
    emb = eng.embed(eng.stft_features(torch.from_numpy(np.concatenate([ca, cb])).to(eng.device),
                                      [0, len(ca), len(ca) + len(cb)], max_frames=spec.NOISE_WIN,
                                      want_phase=False)[0].reshape(2, spec.NOISE_WIN, spec.BINS))
    for S in [int(s) for s in a.streams.split(",")]:
        for H in [int(h) for h in a.hops.split(",")]:
            n = int(round(H * 0.010 * rate_in))
            objs = {}
            for k in ("never", "enabled", "auto") if has else ("never",):
                o = live.LiveSession(eng, S, rate_in, rate_out, 32768, wet=True, lookahead=a.lookahead)
                for i in range(S):
                    o.set_embeddings(i, emb[0], emb[1])
                o.set_wet(0.25)
                if k != "never":
                    o.enable_levels()
                if k == "auto":
                    o.set_auto_wet(200, 1.0)
                objs[k] = o
            pos = {k: 0 for k in objs}

            def push(k):
                i = pos[k] % (len(audio) - n)
                pos[k] += n
                objs[k].push([audio[i:i + n]] * S)

            for k in objs:
                for _ in range(40):
                    push(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in objs}
            for _ in range(a.pushes):
                for k in objs:
                    ts[k].append(_timed(lambda: push(k)))
            launches, level_ms = {}, {}
            for k in objs:
                eng.set_option("profile", 1)
                eng.profile_reset()
                for _ in range(10):
                    push(k)
                prof = eng.profile()
                eng.set_option("profile", 0)
                launches[k] = sum(v["calls"] for v in prof.values()) / 10
                level_ms[k] = round(prof["live_level"]["ms"] / 10, 4) if "live_level" in prof else 0.0
            for o in objs.values():
                o.close()
            line = {"mode": "levels", "streams": S, "hops_per_push": H, "push_audio_ms": H * 10, "pushes": a.pushes,
                    "in_rate": rate_in, "out_rate": rate_out, "lookahead": a.lookahead}
            for k in ("never", "enabled", "auto"):
                line["push_ms_p50_" + k] = pct(ts.get(k, []), 50)
                line["push_ms_p99_" + k] = pct(ts.get(k, []), 99)
                line["launches_per_push_" + k] = launches.get(k)
                line["live_level_ms_per_push_" + k] = level_ms.get(k)
            line.update({"lib": os.path.basename(os.environ.get("NHANS_LIB") or "tree"), "precision": "f16x3",
                         "weights": "synthetic seed 7"})
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
    eng.close()
    return 0


def fullband(a):
    """--fullband: what the full band (nhans_fullband_*) costs a live push.  Per (S, H) one line with mode "fullband": push
    p50 / p99 of two S-slot live.LiveSession objects (48 kHz int16 in and out, mixed round trip, wet 0.25) pushed by turns
    -- "never" (no full-band call at all) and "enabled" (enable_fullband(), gain 1) --, launches per push, and the device
    time of live_out and live_hold per push from a profiled pass of 10.  A library without the feature ($NHANS_LIB)
    reports "never" alone."""
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    rate = a.in_rate or 48000
    idx = (np.arange(int(30.0 * rate)) * float(spec.FS) / rate).astype(np.int64)
    audio = synth.mixture(1, 30.0)[np.minimum(idx, int(30.0 * spec.FS) - 1)]
    has = hasattr(hip.load(), "nhans_fullband_live_enable")
    out = open(a.out, "a") if a.out else None
    pct = lambda v, q: round(float(np.percentile(v, q)), 3) if len(v) else None
    emb = eng.embed(eng.stft_features(torch.from_numpy(np.concatenate([ca, cb])).to(eng.device),
                                      [0, len(ca), len(ca) + len(cb)], max_frames=spec.NOISE_WIN,
                                      want_phase=False)[0].reshape(2, spec.NOISE_WIN, spec.BINS))
    for S in [int(s) for s in a.streams.split(",")]:
        for H in [int(h) for h in a.hops.split(",")]:
            n = int(round(H * 0.010 * rate))
            objs = {}
            for k in ("never", "enabled") if has else ("never",):
                o = live.LiveSession(eng, S, rate, rate, 32768, wet=True, lookahead=a.lookahead)
                for i in range(S):
                    o.set_embeddings(i, emb[0], emb[1])
                o.set_wet(0.25)
                if k == "enabled":
                    o.enable_fullband()
                objs[k] = o
            pos = {k: 0 for k in objs}

            def push(k):
                i = pos[k] % (len(audio) - n)
                pos[k] += n
                objs[k].push([audio[i:i + n]] * S)

            for k in objs:
                for _ in range(40):
                    push(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in objs}
            for _ in range(a.pushes):
                for k in objs:
                    ts[k].append(_timed(lambda: push(k)))
            line = {"mode": "fullband", "streams": S, "hops_per_push": H, "push_audio_ms": H * 10, "pushes": a.pushes, "rate": rate,
                    "lookahead": a.lookahead}
            for k in objs:
                eng.set_option("profile", 1)
                eng.profile_reset()
                for _ in range(10):
                    push(k)
                prof = eng.profile()
                eng.set_option("profile", 0)
                line["push_ms_p50_" + k] = pct(ts[k], 50)
                line["push_ms_p99_" + k] = pct(ts[k], 99)
                line["launches_per_push_" + k] = sum(v["calls"] for v in prof.values()) / 10
                for name in ("live_in", "live_out", "live_hold"):
                    line[name + "_ms_per_push_" + k] = round(prof[name]["ms"] / 10, 4) if name in prof else 0.0
            for o in objs.values():
                o.close()
            line.update({"lib": os.path.basename(os.environ.get("NHANS_LIB") or "tree"), "precision": "f16x3",
                         "weights": "synthetic seed 7"})
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
    eng.close()
    return 0


def interleaved(a):
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    rate_in, rate_out = a.in_rate or 48000, a.out_rate or 48000
    idx = (np.arange(int(30.0 * rate_in)) * float(spec.FS) / rate_in).astype(np.int64)
    audio = synth.mixture(1, 30.0)[np.minimum(idx, int(30.0 * spec.FS) - 1)]
    stereo = np.ascontiguousarray(np.stack([audio, audio[::-1]], axis=1))
    has = hasattr(hip.load(), "nhans_interleaved_live_push")
    out = open(a.out, "a") if a.out else None
    pct = lambda v, q: round(float(np.percentile(v, q)), 3) if len(v) else None
    emb = eng.embed(eng.stft_features(torch.from_numpy(np.concatenate([ca, cb])).to(eng.device),
                                      [0, len(ca), len(ca) + len(cb)], max_frames=spec.NOISE_WIN,
                                      want_phase=False)[0].reshape(2, spec.NOISE_WIN, spec.BINS))
    for S in [int(s) for s in a.streams.split(",")]:
        if S % 2:
            raise SystemExit("--interleaved: an even number of slots (a split stereo stream has two)")
        for H in [int(h) for h in a.hops.split(",")]:
            n = int(round(H * 0.010 * rate_in))
            kinds = {"mono": dict(nslots=S), "downmix": dict(nslots=S, channels=2), "split": dict(nslots=S // 2, channels=2, channel_mode="split")}
            objs = {}
            for k in kinds if has else ("mono",):
                kw = dict(kinds[k])
                o = live.LiveSession(eng, kw.pop("nslots"), rate_in, rate_out, 32768, lookahead=a.lookahead, **kw)
                for i in range(o.S):
                    o.set_embeddings(i, emb[0], emb[1])
                objs[k] = o
            pos = {k: 0 for k in objs}

            def push(k):
                i = pos[k] % (len(audio) - n)
                pos[k] += n
                objs[k].push([audio[i:i + n]] * S if k == "mono" else [stereo[i:i + n]] * (S if k == "downmix" else S // 2))

            for k in objs:
                for _ in range(40):
                    push(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in objs}
            for _ in range(a.pushes):
                for k in objs:
                    ts[k].append(_timed(lambda: push(k)))
            launches, stage_ms = {}, {}
            for k in objs:
                eng.set_option("profile", 1)
                eng.profile_reset()
                for _ in range(10):
                    push(k)
                prof = eng.profile()
                eng.set_option("profile", 0)
                launches[k] = sum(v["calls"] for v in prof.values()) / 10
                stage_ms[k] = {st: round(prof[st]["ms"] / max(prof[st]["calls"], 1), 4) if st in prof else None for st in ("live_in", "live_out")}
            for o in objs.values():
                o.close()
            line = {"mode": "interleaved", "slots": S, "hops_per_push": H, "push_audio_ms": H * 10, "pushes": a.pushes,
                    "in_rate": rate_in, "out_rate": rate_out, "lookahead": a.lookahead}
            for k in kinds:
                line["push_ms_p50_" + k] = pct(ts.get(k, []), 50)
                line["push_ms_p99_" + k] = pct(ts.get(k, []), 99)
                line["launches_per_push_" + k] = launches.get(k)
                line["live_in_ms_" + k] = stage_ms.get(k, {}).get("live_in")
                line["live_out_ms_" + k] = stage_ms.get(k, {}).get("live_out")
            line.update({"lib": os.path.basename(os.environ.get("NHANS_LIB") or "tree"), "precision": "f16x3",
                         "weights": "synthetic seed 7"})
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
    eng.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--churn", action="store_true", help="slots that callers join and leave (see the top of this file)")
    ap.add_argument("--slots", default="64,256")
    ap.add_argument("--active", type=int, default=16)
    ap.add_argument("--every", type=int, default=8, help="--churn: one stream leaves and one joins every this many pushes")
    ap.add_argument("--out", default=None, help="--churn: also append the JSON lines to this file")
    ap.add_argument("--streams", default="1,8,64,256")
    ap.add_argument("--hops", default="1,4,16")
    ap.add_argument("--pushes", type=int, default=60, help="timed pushes per shape (after 40 warm-up pushes)")
    ap.add_argument("--in_rate", type=int, default=None, help="pieces arrive as int16 at this rate (default: 16 kHz float32)")
    ap.add_argument("--out_rate", type=int, default=None, help="pieces are returned at this rate (default: 16 kHz)")
    ap.add_argument("--live", action="store_true", help="drive a live.LiveSession (needs --in_rate and --out_rate)")
    ap.add_argument("--lookahead", type=int, default=spec.LOOKAHEAD, help="look-ahead L of every stream, 0 ... 17 frames")
    ap.add_argument("--capture", action="store_true", help="cost of the sample history and of a capture (see the top of this file)")
    ap.add_argument("--captures", type=int, default=20, help="--capture: timed capture_context / set_context calls")
    ap.add_argument("--levels", action="store_true", help="cost of the level meter and the automatic wet factor (see the top of this file)")
    ap.add_argument("--fullband", action="store_true", help="cost of the full band of a live session per push (see fullband())")
    ap.add_argument("--fbank", action="store_true", help="cost of an attached filterbank per push, and the offline kernel's bytes/s")
    ap.add_argument("--interleaved", action="store_true", help="cost of interleaved stereo frames beside mono slots (see the top of this file)")
    a = ap.parse_args()
    if a.interleaved:
        return interleaved(a)
    if a.fbank:
        return fbank_cost(a)
    if a.churn:
        return churn(a)
    if a.fullband:
        return fullband(a)
    if a.levels:
        return levels(a)
    if a.capture:
        return capture(a)
    if a.live and not (a.in_rate and a.out_rate):
        ap.error("--live needs --in_rate and --out_rate")
    if not 0 <= a.lookahead <= spec.LOOKAHEAD:
        ap.error("--lookahead is 0 ... %d frames" % spec.LOOKAHEAD)
    out = open(a.out, "a") if a.out else None
    eng = engine.Engine("denoiser", precision="f16x3")
    ca, cb = apply.normalise(synth.silent()), apply.normalise(synth.noise_context(1))
    audio = apply.normalise(synth.mixture(1, 30.0))
    lat = online.latency_ms(in_rate=a.in_rate, out_rate=a.out_rate, lookahead=a.lookahead)
    rates = {}
    if a.in_rate or a.out_rate:
        rates = {"in_rate": a.in_rate, "out_rate": a.out_rate}
    if a.in_rate:
        # the same recording held at the input rate (nearest sample), as int16 with a fixed peak
        idx = (np.arange(int(30.0 * a.in_rate)) * float(spec.FS) / a.in_rate).astype(np.int64)
        audio = synth.mixture(1, 30.0)[np.minimum(idx, int(30.0 * spec.FS) - 1)]
        rates["peak"] = 32768
    for S in [int(s) for s in a.streams.split(",")]:
        for H in [int(h) for h in a.hops.split(",")]:
            n = H * spec.HOP if not a.in_rate else int(round(H * 0.010 * a.in_rate))
            if a.live:
                enh = live.LiveSession(eng, S, a.in_rate, a.out_rate, rates["peak"], lookahead=a.lookahead)
                # (one tower run; every slot gets its rows)
                emb = eng.embed(eng.stft_features(torch.from_numpy(np.concatenate([ca, cb])).to(eng.device),
                                                  [0, len(ca), len(ca) + len(cb)], max_frames=spec.NOISE_WIN,
                                                  want_phase=False)[0].reshape(2, spec.NOISE_WIN, spec.BINS))
                for i in range(S):
                    enh.set_embeddings(i, emb[0], emb[1])
            else:
                enh = online.OnlineEnhancer(eng, [ca] * S, [cb] * S, lookahead=a.lookahead, **rates)
            pos = [0]

            def push():
                i = pos[0] % (len(audio) - n)
                pos[0] += n
                enh.push([audio[i:i + n]] * S)

            for _ in range(40):              # past the look-ahead (17 frames at most): every push then runs the whole path
                push()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.pushes):
                t0 = time.perf_counter()
                push()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            eng.set_option("profile", 1)
            eng.profile_reset()
            for _ in range(10):
                push()
            prof = eng.profile()
            eng.set_option("profile", 0)
            enh.close()
            kern = sum(v["ms"] for v in prof.values()) / 10
            p50, p99 = float(np.percentile(ts, 50)), float(np.percentile(ts, 99))
            line = json.dumps({"mode": "live" if a.live else "online", "streams": S, "hops_per_push": H,
                               "push_audio_ms": H * 10, "push_ms_p50": round(p50, 3),
                               "push_ms_p99": round(p99, 3), "kernel_ms_per_push": round(kern, 3),
                               "launches_per_push": sum(v["calls"] for v in prof.values()) / 10,
                               "realtime_factor": round(S * H * 0.010 / (p50 / 1e3), 2),
                               "lookahead": a.lookahead, "latency_ms": [lat[0], lat[1]],
                               "lib": os.path.basename(os.path.dirname(os.environ["NHANS_LIB"])) if os.environ.get("NHANS_LIB") else "tree",
                               "precision": "f16x3", "weights": "synthetic seed 7",
                               **{k: v for k, v in rates.items() if k != "peak"}})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
